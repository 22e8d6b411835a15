"""Length control and logit bias on the MI355X: the PN sampler instantiations with a length record, a decay table and a bias table over
given logits (dtk_op_sample_shape) in the three sampler families against tests/shape_oracle.py, the off path, one sequence end to end
over the device's own logits with the bias table read back, batched steps of the multi-vector and the MFMA family driven from the host
and by both engines, the thresholds across dtk_kv_fork / dtk_resume_slot, and the reset of dtk_set_sampling_slot."""
from __future__ import annotations

import ctypes as C
import gc
import threading

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from detikzify_amd.model.modeling import dry_struct, length_struct
from oracle import sampling
from oracle.ops import rb
from tests import shape_oracle
from tests.helpers import TINY, sketch_image
from tests.test_gpu_penalty import _oracle_row, _raw_lse, _set
from tests.test_gpu_trunc import FAMILIES, _bigvocab

pytestmark = pytest.mark.gpu

BAD, BEGIN, SEED = [1], [2], 4711
DRAWS = 5
I64P, I32P, F32P = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def big():
    m = _bigvocab()
    m.enable_logprobs()
    yield m
    del m
    gc.collect()


def _i64(ids):
    a = np.asarray(list(ids), dtype=np.int64)
    return a, a.ctypes.data_as(I64P)


def _pairs(pairs):
    ids = np.asarray([t for t, _ in pairs] or [0], dtype=np.int32)
    vals = np.asarray([v for _, v in pairs] or [0.0], dtype=np.float32)
    return ids, vals, ids.ctypes.data_as(I32P), vals.ctypes.data_as(F32P), len(pairs)


# ------------------------------------------------------------------------------------------ the samplers with the tables
# the op-level rows run over FAMILIES and two more load-site forms with every table on: k_sample's 16-byte pass 1 (V % 4 == 0; at 32 769 it
# runs scalar) and a sampling row over the chain's ragged tail (the last slice ends inside a thread's 8 ids, 3 of them valid; at 40 000
# every thread is full, at 32 769 only greedy rows reach the chain).  Both below the fixture's vocabulary: probs_out is allowed
OP_V = {**FAMILIES, 36864: "k_sample-16B", 36867: "k_smb_*-ragged"}
TOPK_V = (32769, 36864)          # the vocabularies whose sampling rows ask top_k = V - 1: k_sample
START = 5          # length_start of every op-level row
MIN_NEW, DSTART = 4, 6


def _rows(V):
    """(tag, logits, config, shape, moves): shape = the oracle's arguments (cur, eos, min_new, decay, pairs, counted, pp, fp, h, dry_m),
    moves = whether the transformed row must differ from the raw one.  EOS ids 0, V - 2 and V - 1; biased ids in the last 8 columns (the
    ragged tail of mb_load at 32 769: id 32 768 alone) and 256 of them in one row; n = cur - START on both sides of both thresholds; k at
    the 2^100 clamp.  Which kernels a row runs is the launchers' rule (tests/test_gpu_penalty.py::_rows): everything k_sample_fast at
    32 000; above 32 768 a sampling row with 0 < top_k < V (TOPK_V) runs k_sample, and a row with top_k = 0 or a greedy one the chain."""
    g = torch.Generator().manual_seed(V + 23)
    nk = V - 1 if V in TOPK_V else 0
    wide = lambda: rb(torch.randn(V, generator=g) * 4)
    E = [0, V - 2, V - 1]
    S = dict(do_sample=True, temperature=1.1, top_k=nk, top_p=0.9, min_p=0.05, eps=3e-4)
    GREEDY = dict(do_sample=False, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, eps=0.0)
    eosy = wide().clone()
    eosy[E] = eosy.max() - torch.tensor([0.25, 0.5, 0.0])          # the EOS ids carry mass: positive logits near the top
    negy = wide().clone()
    m = float(negy.max())
    negy[0], negy[V - 2], negy[V - 1] = -m, 0.0, m - 0.5             # a negative EOS logit and one of exactly 0
    last8 = [(V - 8 + i, v) for i, v in enumerate((3.0, -2.5, 0.75, 100.0, -100.0, 1e-3, -4.0, 2.0))]
    last8[3] = (V - 5, 6.0)
    rs = np.random.default_rng(V)
    must = sorted(set([0, 1, 8191, 8192, V - 1, V - 2, (V - 1) // 8 * 8] + torch.topk(eosy, 40)[1].tolist()[:30]))
    rest = [int(t) for t in rs.permutation(V) if int(t) not in set(must)]
    many_ids = sorted(must + rest[:256 - len(must)])
    many = [(int(t), float(np.float32(rs.uniform(-5, 5)))) for t in many_ids]
    assert len(many) == 256
    allon = wide().clone()
    allon[E] = allon.max() - torch.tensor([1.0, 2.0, 0.5])
    t6 = torch.topk(allon, 6)[1].tolist()
    hist = [31, 32, t6[0], 33, 31, 32]                               # DRY: t6[0] would extend a repetition of length 2
    sh = lambda cur, **kw: dict(cur=cur, eos=E, start=START, **kw)
    gmin = wide().clone()
    gmin[V - 1] = gmin.max() + 1.0                                   # the raw arg-max is an EOS id
    gbias = wide().clone()
    rows = [("min: n = min_new - 1", eosy, S, sh(START + MIN_NEW - 1, min_new=MIN_NEW, decay=(DSTART, 1.3)), True),
            ("min: n = min_new", eosy, S, sh(START + MIN_NEW, min_new=MIN_NEW, decay=(DSTART, 1.3)), False),
            ("decay: n = decay_start", eosy, S, sh(START + DSTART, min_new=MIN_NEW, decay=(DSTART, 1.3)), False),
            ("decay: n = decay_start + 1", eosy, S, sh(START + DSTART + 1, min_new=MIN_NEW, decay=(DSTART, 1.3)), True),
            ("decay: negative and zero EOS logits, factor 0.9", negy, S, sh(START + DSTART + 9, decay=(DSTART, 0.9)), True),
            ("decay: k at the clamp", negy, S, sh(START + DSTART + 140, decay=(DSTART, 2.0)), True),
            ("bias: last 8 columns", eosy, S, sh(START + 1, pairs=dict(last8)), True),
            ("bias: 256 ids + min", eosy, S, sh(START + 1, min_new=MIN_NEW, pairs=dict(many)), True),
            ("all on: bias, pair, DRY, decay", allon, S,
             sh(START + DSTART + 3, min_new=MIN_NEW, decay=(DSTART, 1.3), pairs={t6[1]: -1.5, V - 1: 0.5, t6[2]: 0.25},
                counted=[t6[1], t6[1], V - 1], pp=0.6, fp=0.4, h=hist, dry_m=0.8), True),
            ("greedy: min holds the arg-max back", gmin, GREEDY, sh(START + 1, min_new=MIN_NEW), True),
            ("greedy: a bias in the last column group lifts an id", gbias, GREEDY, sh(START + 1, pairs={V - 3: 40.0}), True),
            ("greedy: decay at the clamp", negy, GREEDY, sh(START + DSTART + 101, decay=(DSTART, 2.0)), True)]
    return rows


def _device_args(shape, V):
    """the C arguments of one row's shape"""
    l = length_struct(shape.get("min_new", 0), shape.get("decay"), shape["start"], shape["eos"])
    d = dry_struct(shape.get("dry_m", 0.0), 1.75, 2, 0, ())
    pairs = sorted(shape.get("pairs", {}).items())
    return l, d, _pairs(pairs), _i64(shape.get("counted", ())), _i64(shape.get("h", ()))


@pytest.mark.parametrize("V", list(OP_V), ids=[f"{v}-{k}" for v, k in OP_V.items()])
def test_op_sample_shape_matches_the_oracle(big, V):
    """every draw: the token is the oracle's over the transformed row z'; the token, probs_out and sample_logprob are, bit for bit, what
    the same kernels give for the oracle's z' handed in as the row (dtk_op_sample_ext: everything behind the load sites is a function of
    z' alone); logprob is the bits of fp32(z[t] - L) over the RAW row, L read off dtk_op_sample_lp (tests/test_gpu_penalty.py::_raw_lse)"""
    model = big
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    tok, tok2, lp, lp2 = C.c_int64(), C.c_int64(), (C.c_float * 2)(), (C.c_float * 2)()
    probs, probs2 = np.empty(V, dtype=np.float32), np.empty(V, dtype=np.float32)
    n_rows = 0
    for tag, logits, cfg, shape, moves in _rows(V):
        n_rows += 1
        lb = logits.numpy().copy()
        l, d, (bi, bv, bip, bvp, nb), (ca, cp), (ha, hp) = _device_args(shape, V)
        pp, fp = shape.get("pp", 0.0), shape.get("fp", 0.0)
        _set(model, cfg)
        x = _lib.DtkSamplingExt(min_p=cfg["min_p"], epsilon_cutoff=cfg["eps"])
        zp = shape_oracle.transform(logits, **shape)
        same = bool(torch.equal(zp.view(torch.int32), logits.view(torch.int32)))
        assert same != moves, (V, tag)
        zb = zp.numpy().copy()
        L = _raw_lse(model, lb, logits, V, 8)
        assert L is not None, (V, tag, "no draw of dtk_op_sample_lp gives the raw logsumexp exactly")
        lp_bits = lambda t: bytes(C.c_float(float(np.float32(np.float32(float(logits[t])) - L))))
        call = lambda n, t, pr, lo: model._check(model.lib.dtk_op_sample_shape(
            model._ctx, ptr(lb), V, n, C.byref(t), pr, lo, C.byref(x), pp, fp, cp, len(ca), hp, len(ha), C.byref(d),
            shape["cur"], C.byref(l), bip, bvp, nb), "dtk_op_sample_shape")
        ref_call = lambda n: model._check(model.lib.dtk_op_sample_ext(model._ctx, ptr(zb), V, n, C.byref(tok2), ptr(probs2), lp2, C.byref(x)),
                                          "dtk_op_sample_ext")
        if not cfg["do_sample"]:
            want, raw = sampling.greedy(zp, BAD, BEGIN, True), sampling.greedy(logits, BAD, BEGIN, True)
            assert want != raw, (V, tag)               # the row shows something: the rule moves the arg-max
            call(0, tok, ptr(probs), lp)
            assert tok.value == want and probs[want] == 1.0 and int((probs != 0).sum()) == 1, (V, tag, tok.value, want)
            assert bytes(C.c_float(lp[0])) == lp_bits(want) and lp[1] == 0.0, (V, tag, lp[0], lp[1])
            call(0, tok, None, None)
            assert tok.value == want
            continue
        ref = {first: _oracle_row(zp, cfg, first) for first in (True, False)}
        if moves:
            assert not torch.equal(ref[False][0], _oracle_row(logits, cfg, False)[0]), (V, tag, "the rule does not move the kept masses")
        for n in range(DRAWS):
            qk, total, run = ref[n == 0]
            target = (total * sampling.rand32(SEED, n)) >> 32
            want = int(torch.searchsorted(run, torch.tensor(target, dtype=torch.int64), right=True))
            call(n, tok, ptr(probs), lp)
            t = tok.value
            assert t == want, (V, tag, n, t, want)
            ref_call(n)
            assert tok2.value == t and probs.tobytes() == probs2.tobytes(), (V, tag, n)
            assert bytes(C.c_float(lp[1])) == bytes(C.c_float(lp2[1])), (V, tag, n, lp[1], lp2[1])
            assert bytes(C.c_float(lp[0])) == lp_bits(t), (V, tag, n, lp[0])
            if n % 3 == 0:      # the kernels without the log-probability code: the same token
                call(n, tok2, None, None)
                assert tok2.value == t, (V, tag, n)
    assert n_rows == 12


@pytest.mark.parametrize("V", list(OP_V), ids=[f"{v}-{k}" for v, k in OP_V.items()])
def test_off_means_off_at_op_level(big, V):
    """no rule and no bias (a record that is all off, at a length far beyond every threshold): the token, the probabilities and both
    log-probabilities of dtk_op_sample_ext, bit for bit; likewise rules without an EOS id, and a bias table of zeros"""
    model = big
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    logits = rb(torch.randn(V, generator=torch.Generator().manual_seed(V + 1)) * 4)
    lb = logits.numpy().copy()
    d = dry_struct(0.0, 1.75, 1, 0)
    tok, tok2, lp, lp2 = C.c_int64(), C.c_int64(), (C.c_float * 2)(), (C.c_float * 2)()
    p1, p2 = np.empty(V, dtype=np.float32), np.empty(V, dtype=np.float32)
    offs = [(length_struct(0, None, 0, ()), []), (length_struct(50, (60, 2.0), 0, ()), []), (length_struct(0, None, 3, (0, V - 1)), [(V - 1, 0.0), (7, -0.0)])]
    for T, k, p, mp, eps in ((0.8, V - 1 if V in TOPK_V else 0, 0.95, 0.0, 0.0), (1.3, 50, 1.0, 0.1, 3e-4)):
        model.set_sampling(do_sample=True, temperature=T, top_p=p, top_k=k, seed=SEED, bad_ids=BAD, begin_suppress_ids=BEGIN)
        x = _lib.DtkSamplingExt(min_p=mp, epsilon_cutoff=eps)
        for l, pairs in offs:
            bi, bv, bip, bvp, nb = _pairs(pairs)
            for n in range(3):
                model._check(model.lib.dtk_op_sample_shape(model._ctx, ptr(lb), V, n, C.byref(tok), ptr(p1), lp, C.byref(x), 0.0, 0.0, None, 0,
                                                           None, 0, C.byref(d), 40, C.byref(l), bip, bvp, nb), "dtk_op_sample_shape")
                model._check(model.lib.dtk_op_sample_ext(model._ctx, ptr(lb), V, n, C.byref(tok2), ptr(p2), lp2, C.byref(x)), "dtk_op_sample_ext")
                assert tok.value == tok2.value and p1.tobytes() == p2.tobytes() and bytes(lp) == bytes(lp2), (V, T, k, n)
    # the ranges: DTK_ERR_ARG, nothing launched
    ok_l, (bi, bv, bip, bvp, nb) = length_struct(2, (3, 1.5), 0, (0,)), _pairs([(3, 1.0)])
    call = lambda l, ids, vals, n: model.lib.dtk_op_sample_shape(model._ctx, ptr(lb), V, 0, C.byref(tok), None, None, None, 0.0, 0.0, None, 0, None, 0,
                                                                 C.byref(d), 9, C.byref(l), ids, vals, n)
    assert call(ok_l, bip, bvp, nb) == 0
    for bad in (length_struct(-1, None, 0, (0,)), length_struct(0, (-1, 1.5), 0, (0,)), length_struct(0, (0, -1.5), 0, (0,)),
                length_struct(0, (0, float("nan")), 0, (0,)), length_struct(0, (0, float("inf")), 0, (0,)), length_struct(4, (3, 1.5), 0, (0,)),
                length_struct(2, None, -1, (0,)), length_struct(2, None, 0, (V,)), length_struct(2, None, 0, (-1,))):
        assert call(bad, bip, bvp, nb) == -1
        if bad.eos_ids[0] != V:          # (an op-level V below the context's own vocabulary is a valid id of the context)
            assert model.lib.dtk_set_length_control(model._ctx, C.byref(bad)) == -1
    over = length_struct(2, None, 0, (0,))
    over.n_eos = 9
    assert call(over, bip, bvp, nb) == -1 and model.lib.dtk_set_length_control(model._ctx, C.byref(over)) == -1
    for pairs in ([(V, 1.0)], [(-1, 1.0)], [(3, 100.5)], [(3, float("nan"))], [(3, float("-inf"))], [(3, 1.0), (3, 2.0)]):
        bi, bv, bip, bvp, nb = _pairs(pairs)
        assert call(ok_l, bip, bvp, nb) == -1, pairs
    bi, bv, bip, bvp, nb = _pairs([(t, 1.0) for t in range(257)])
    assert call(ok_l, bip, bvp, nb) == -1 and model.lib.dtk_set_logit_bias(model._ctx, bip, bvp, nb) == -1


# ------------------------------------------------------------------------------------------ one sequence, end to end
TAIL = [77, 30, 9, 41, 30, 9]
EOSID = 3          # the sequences' EOS id in these tests: a plain text token of the toy vocabularies
LIFT = 30.0        # a bias that makes an id certain on the toys' flat logits


def _single(name):
    if name == "detikzify-tiny":
        from detikzify_amd.model import load
        model, proc = load(name, synthetic=1234)
        enc = proc(images=sketch_image(2, 96), return_tensors="pt")
        base, px, img = enc.input_ids[0], enc.pixel_values, TINY.image_token_id
    else:
        model = _bigvocab()
        cfg = model.config
        base, px, img = torch.tensor([cfg.image_token_id] * cfg.num_patches), torch.zeros(1, 3, cfg.vit_image, cfg.vit_image), cfg.image_token_id
    return model, torch.cat([base, torch.tensor(TAIL, dtype=torch.int64)]), px, img, int(base.numel())


def _by_hand(model, ids, px, img, cfg, seed, n_max, eos, **shape):
    """the sequence stepped by hand: every token against the oracle's pick over the row the device sampled from; stops behind an EOS.
    shape: min_new, decay, start, pairs.  Returns (tokens, steps on which the pick over the raw row is another token)"""
    T = int(ids.numel())
    model.set_sampling(do_sample=cfg["do_sample"], temperature=cfg["temperature"], top_p=cfg["top_p"], seed=seed, bad_ids=[img])
    model.set_length_control(shape.get("min_new", 0), shape.get("decay"), shape.get("start", T), eos)
    model.set_logit_bias(shape.get("pairs"))
    model.prefill(ids, px)
    made, moved = [], 0
    okw = dict(eos=eos, min_new=shape.get("min_new", 0), decay=shape.get("decay"), start=shape.get("start", T), pairs=shape.get("pairs"))
    for n in range(n_max):
        row = model.get_logits()
        model.decode_launch()
        tok = model.decode_wait()
        if cfg["do_sample"]:
            want = shape_oracle.draw(row, T + n, cfg["temperature"], 0, cfg["top_p"], seed, n, bad=[img], **okw)[0]
            raw = shape_oracle.draw(row, T + n, cfg["temperature"], 0, cfg["top_p"], seed, n, bad=[img])[0]
        else:
            want, raw = shape_oracle.greedy(row, T + n, bad=[img], **okw), shape_oracle.greedy(row, T + n, bad=[img])
        assert tok == want, (n, tok, want)
        moved += want != raw
        made.append(tok)
        if tok in eos:
            break
    return made, moved


@pytest.mark.parametrize("name", ["detikzify-tiny", "tiny-v2-40000"])
def test_generate_is_the_oracle_over_the_device_logits(name):
    """k_sample_fast on the toy vocabulary, the multi-block chain at 40 000.  With a bias that makes EOS certain, min_new_tokens holds it
    back until exactly token min_new; with factor 2.0 the decay ends the program where the oracle, run over the device's own per-step
    logits, says it ends; the bias table is read back; a later plain call is the plain run again"""
    model, ids, px, img, S = _single(name)
    T, V = int(ids.numel()), int(model.config.vocab)
    SAMPLE = dict(do_sample=True, temperature=1.0, top_p=0.95)
    GEN = dict(input_ids=ids[None], pixel_values=px, max_new_tokens=40, eos_token_id=EOSID, bad_words_ids=[[img]], seed=31, do_sample=True,
               temperature=1.0, top_p=0.95, top_k=0)
    assert int(model.logit_bias_table().count_nonzero()) == 0
    plain = model.generate(**GEN)[0, T:].tolist()
    assert model.generate(min_new_tokens=0, exponential_decay_length_penalty=None, logit_bias={}, **GEN)[0, T:].tolist() == plain
    assert model.generate(min_new_tokens=7, **{**GEN, "eos_token_id": -1})[0, T:].tolist() == model.generate(**{**GEN, "eos_token_id": -1})[0, T:].tolist()
    # 1. EOS is certain (+30 on flat logits) and held back: tokens 0 .. min_new - 1 are no EOS, token min_new is
    MIN = 6
    bias = {EOSID: LIFT, V - 1: -2.0, 8: 0.5}
    held = model.generate(min_new_tokens=MIN, logit_bias=bias, **GEN)[0, T:].tolist()
    assert len(held) == MIN + 1 and held[-1] == EOSID and EOSID not in held[:-1], held
    tab = model.logit_bias_table()
    assert int(tab.count_nonzero()) == 3 and tab[EOSID] == LIFT and tab[V - 1] == -2.0 and tab[8] == 0.5
    hand, moved = _by_hand(model, ids, px, img, SAMPLE, 31, 40, (EOSID,), min_new=MIN, pairs=bias)
    assert hand == held and moved >= 1
    # ... counted from length_start: the whole text behind the image prompt counts, so EOS comes MIN - len(TAIL) tokens in ... = at once
    early = model.generate(min_new_tokens=MIN, length_start=S, logit_bias=bias, **GEN)[0, T:].tolist()
    assert early == [EOSID]
    # greedy takes the rules as well
    gheld = model.generate(min_new_tokens=3, logit_bias=bias, **{**GEN, "do_sample": False})[0, T:].tolist()
    assert len(gheld) == 4 and gheld[-1] == EOSID and EOSID not in gheld[:-1]
    # 2. the decay alone (factor 2.0 from token 4 on) ends the program within the steps the oracle predicts
    DEC = (4, 2.0)
    dec = model.generate(exponential_decay_length_penalty=DEC, **GEN)[0, T:].tolist()
    hand, moved = _by_hand(model, ids, px, img, SAMPLE, 31, 40, (EOSID,), decay=DEC)
    assert hand == dec and dec[-1] == EOSID and len(dec) < 40 and moved >= 1, (dec, moved)
    print(f"{name}: min_new_tokens = {MIN} ends at token {len(held) - 1}; decay {DEC} ends at token {len(dec) - 1} (plain: {len(plain)} tokens)")
    assert int(model.logit_bias_table().count_nonzero()) == 0                           # (the last setter cleared the table: its ids re-zeroed)
    # refused while a step is unread (DTK_ERR_STATE), and nothing changes
    model.set_sampling(do_sample=False, bad_ids=[img])
    model.prefill(ids, px)
    model.decode_launch()
    l = length_struct(2, None, 0, (EOSID,))
    bi, bv, bip, bvp, nb = _pairs([(3, 1.0)])
    assert model.lib.dtk_set_length_control(model._ctx, C.byref(l)) == -3 and model.lib.dtk_set_logit_bias(model._ctx, bip, bvp, nb) == -3
    model.decode_wait()
    # a later plain call is the plain run again, and set_sampling reset the table
    model.set_logit_bias(bias)
    assert int(model.logit_bias_table().count_nonzero()) == 3
    assert model.generate(**GEN)[0, T:].tolist() == plain
    assert int(model.logit_bias_table().count_nonzero()) == 0
    del model
    gc.collect()


# ------------------------------------------------------------------------------------------ batched steps
# slot s: (min_new_tokens, decay, bias pairs); length_start: the prompt's length
SETS = [(5, None, {EOSID: LIFT}), (0, None, {}), (2, (2, 2.0), {41: 2.0, 60: -3.0}), (0, None, {t: (1.5 if t % 2 else -1.5) for t in range(100, 356)})]
STEPS = 12
TEMP = 1.0


def _prompts(proc, n):
    enc = proc(images=sketch_image(5, 96), return_tensors="pt")
    base, px = enc.input_ids[0], enc.pixel_values
    tails = [[20 + s, 41 + s, 20 + s, 41 + s, 60, 20 + s][:4 + s % 3] for s in range(n)]
    return [torch.cat([base, torch.tensor(t, dtype=torch.int64)]) for t in tails], px, int(base.numel())


def _apply(model, s, T):
    m, decay, pairs = SETS[s]
    model.set_sampling(slot=s, do_sample=True, temperature=TEMP, seed=900 + s, bad_ids=[TINY.image_token_id])
    if m or decay:
        model.set_length_control(m, decay, T, (EOSID,), slot=s)
    if pairs:
        model.set_logit_bias(pairs, slot=s)


def _drive(model, prompts, px, slots, check, shaped=None):
    """STEPS batched steps of `slots` driven from the host (a slot goes on behind its EOS: the device does not care); check: every token
    against the oracle's draw over the slot's own logits.  shaped: the slots that get their values (default: all)"""
    shaped = slots if shaped is None else shaped
    for s in slots:
        if s in shaped:
            _apply(model, s, int(prompts[s].numel()))
        else:
            model.set_sampling(slot=s, do_sample=True, temperature=TEMP, seed=900 + s, bad_ids=[TINY.image_token_id])
        model.prefill(prompts[s], px, slot=s)
    toks = {s: [] for s in slots}
    for n in range(STEPS):
        rows = {s: model.get_logits_slot(s) for s in slots} if check else {}
        model.decode_batch_launch(slots)
        t = model.decode_batch_wait()
        for s in slots:
            if check:
                m, decay, pairs = SETS[s] if s in shaped else (0, None, {})
                T = int(prompts[s].numel())
                want = shape_oracle.draw(rows[s], T + n, TEMP, 0, 1.0, 900 + s, n, bad=[TINY.image_token_id], eos=(EOSID,), min_new=m, decay=decay,
                                         start=T, pairs=pairs)[0]
                assert t[s] == want, (s, n, t[s], want)
            toks[s].append(int(t[s]))
    return toks


def _until_eos(toks):
    return toks[:toks.index(EOSID) + 1] if EOSID in toks else toks


@pytest.fixture(scope="module", params=[5, 17], ids=["mv-4", "mfma-16"])
def batched(request):
    """detikzify-tiny with 5 slots (slots 0..3 decode with the multi-vector kernels) and with 17 (one MFMA column tile)"""
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny", synthetic=1234, batch_slots=request.param)
    assert model.max_decode_slots() == (4 if request.param == 5 else 16)
    prompts, px, S = _prompts(proc, 4)
    hand = _drive(model, prompts, px, [0, 1, 2, 3], check=True)       # (before anything switches the log-probabilities on)
    yield model, prompts, px, S, hand
    del model
    gc.collect()


def test_slots_with_their_own_values_are_exact_and_as_alone(batched):
    model, prompts, px, S, hand = batched
    assert hand[0][5] == EOSID and EOSID not in hand[0][:5]            # slot 0: EOS at exactly token min_new
    assert EOSID in hand[2][3:]                                        # slot 2: the decay brought EOS
    for s in range(4):
        tab = model.logit_bias_table(slot=s)
        assert {int(i): float(tab[i]) for i in tab.nonzero().flatten()} == {k: float(np.float32(v)) for k, v in SETS[s][2].items()}, s
        assert _drive(model, prompts, px, [s], check=False)[s] == hand[s], s
    # the values matter: slot 1 (off) is the plain sampler's sequence, and the other slots' are not what they would be without values
    plain = _drive(model, prompts, px, [0, 1, 2, 3], check=True, shaped=[])
    assert plain[1] == hand[1]
    assert all(int(model.logit_bias_table(slot=s).count_nonzero()) == 0 for s in range(4))          # dtk_set_sampling_slot reset the tables
    assert plain[0] != hand[0] and plain[2] != hand[2] and plain[3] != hand[3]
    # values on slot 0 only: slot 1 draws what it draws alone, and slot 0 what it drew with the others
    got = _drive(model, prompts, px, [0, 1], check=False, shaped=[0])
    assert got[1] == plain[1] and got[0] == hand[0]
    # a slot that is part of an unread step refuses the setters (DTK_ERR_STATE); another slot takes them
    model.decode_batch_launch([0])
    l = length_struct(2, None, 0, (EOSID,))
    bi, bv, bip, bvp, nb = _pairs([(3, 1.0)])
    assert model.lib.dtk_set_length_control_slot(model._ctx, 0, C.byref(l)) == -3 and model.lib.dtk_set_logit_bias_slot(model._ctx, 0, bip, bvp, nb) == -3
    assert model.lib.dtk_set_length_control_slot(model._ctx, 1, C.byref(l)) == 0 and model.lib.dtk_set_logit_bias_slot(model._ctx, 1, bip, bvp, nb) == 0
    model.decode_batch_wait()
    assert model.lib.dtk_set_length_control_slot(model._ctx, 99, C.byref(l)) == -1


@pytest.mark.parametrize("engine", ["native", "python"])
def test_engines_carry_the_values_with_the_joins(batched, engine):
    """four sequences with their own values through either engine: the tokens of the same slots driven by hand (up to their EOS), which
    the fixture checked against the oracle; a later join without values inherits nothing"""
    from detikzify_amd.infer.batching import BatchEngine
    from detikzify_amd.infer.engine import NativeBatchEngine
    model, prompts, px, S, hand = batched
    eng = (NativeBatchEngine if engine == "native" else BatchEngine)(model, max_batch=4, share_prefix=False, resume_in_place=False)
    got, errs = {}, []
    common = dict(pixel_values=px, max_new_tokens=STEPS, eos_token_id=EOSID, bad_words_ids=[[TINY.image_token_id]], do_sample=True,
                  temperature=TEMP, top_k=0)
    vals = lambda s: dict(min_new_tokens=SETS[s][0], exponential_decay_length_penalty=SETS[s][1], logit_bias=SETS[s][2])

    def run(s):
        try:
            got[s] = model.generate(input_ids=prompts[s][None], seed=900 + s, **vals(s), **common)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    try:
        ths = [threading.Thread(target=run, args=(s,)) for s in range(4)]
        [t.start() for t in ths]
        [t.join(timeout=120) for t in ths]
        assert not any(t.is_alive() for t in ths) and not errs, errs[:1]
        again = model.generate(input_ids=prompts[0][None], seed=900, **common)
        again_vals = model.generate(input_ids=prompts[0][None], seed=900, **vals(0), **common)
    finally:
        eng.close()
    T = [p.numel() for p in prompts]
    for s in range(4):
        assert got[s][0, T[s]:].tolist() == _until_eos(hand[s]), (engine, s)
    assert again_vals[0, T[0]:].tolist() == _until_eos(hand[0])
    ref = _until_eos(_drive(model, prompts, px, [0], check=False, shaped=[])[0])
    assert again[0, T[0]:].tolist() == ref and ref != _until_eos(hand[0])      # the join without values is the plain run


# ------------------------------------------------------------------------------------------ the chain, batched
def test_two_slots_of_the_chain_with_their_own_values():
    """the 40 000-token toy with slots: the multi-block chain with a slot offset on the records and the tables (sample_bind_slot) and the length
    read from the snapshot k_smb_max leaves, 9 steps of three slots: a minimum with a certain EOS, a decay with biases in the last 8
    columns, and one without values, which draws what it draws alone.  Every token is the oracle's draw over the slot's own row"""
    model = _bigvocab(slots=4)
    cfg = model.config
    img, P, V = cfg.image_token_id, cfg.num_patches, int(cfg.vocab)
    px = torch.zeros(1, 3, cfg.vit_image, cfg.vit_image)
    prompts = [torch.tensor([img] * P + TAIL), torch.tensor([img] * P + [8192, 39999, 8192]), torch.tensor([img] * P + [7, 8])]
    vals = [(4, None, {EOSID: LIFT, V - 1: 1.0}), (1, (2, 2.0), {V - 8 + i: (-1) ** i * 2.0 for i in range(8)}), (0, None, {})]

    def run(slots, shaped):
        for s in slots:
            model.set_sampling(slot=s, do_sample=True, temperature=1.0, top_p=0.95, seed=500 + s, bad_ids=[img])
            if s in shaped:
                model.set_length_control(vals[s][0], vals[s][1], int(prompts[s].numel()), (EOSID, V - 2), slot=s)
                model.set_logit_bias(vals[s][2], slot=s)
            model.prefill(prompts[s], px, slot=s)
        toks, moved = {s: [] for s in slots}, {s: 0 for s in slots}
        for n in range(9):
            rows = {s: model.get_logits_slot(s) for s in slots}
            model.decode_batch_launch(slots)
            t = model.decode_batch_wait()
            for s in slots:
                m, decay, pairs = vals[s] if s in shaped else (0, None, {})
                T = int(prompts[s].numel())
                want = shape_oracle.draw(rows[s], T + n, 1.0, 0, 0.95, 500 + s, n, bad=[img], eos=(EOSID, V - 2), min_new=m, decay=decay, start=T,
                                         pairs=pairs)[0]
                raw = shape_oracle.draw(rows[s], T + n, 1.0, 0, 0.95, 500 + s, n, bad=[img])[0]
                assert int(t[s]) == want, (s, n, int(t[s]), want)
                moved[s] += want != raw
                toks[s].append(int(t[s]))
        return toks, moved

    toks, moved = run([0, 1, 2], [0, 1])
    print("chain, 3 slots: steps on which the draw over z' is not the raw row's:", moved)
    assert toks[0][4] == EOSID and EOSID not in toks[0][:4] and moved[0] >= 1 and moved[1] >= 1 and moved[2] == 0
    alone, _ = run([2], [])
    assert alone[2] == toks[2]
    tab = model.logit_bias_table(slot=1)
    assert tab[V - 8:].tolist() == [2.0, -2.0] * 4 and int(tab.count_nonzero()) == 8
    del model
    gc.collect()


# ------------------------------------------------------------------------------------------ the thresholds follow the sequence
def test_thresholds_across_fork_and_resume_and_the_reset():
    """a slot forked or resumed at a length just below the minimum crosses it at the right token, with no setter call in between: the
    rules are static and n comes from the slot's own position"""
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny", synthetic=1234, batch_slots=5)
    prompts, px, S = _prompts(proc, 1)
    prompt, img = prompts[0], TINY.image_token_id
    T = int(prompt.numel())
    key = model.image_key(px)
    MIN = (T - S) + 5          # counted from the end of the image prompt: five more tokens behind the prompt
    bias = {EOSID: LIFT}

    def setup(s, seed):
        model.set_sampling(slot=s, do_sample=True, temperature=1.2, seed=seed, bad_ids=[img])
        model.set_length_control(MIN, (MIN + 2, 1.5), S, (EOSID,), slot=s)
        model.set_logit_bias(bias, slot=s)

    def step(slots, cur, seeds, draws):
        rows = {s: model.get_logits_slot(s) for s in slots}
        model.decode_batch_launch(slots)
        t = model.decode_batch_wait()
        for s in slots:
            want = shape_oracle.draw(rows[s], cur[s], 1.2, 0, 1.0, seeds[s], draws[s], bad=[img], eos=(EOSID,), min_new=MIN, decay=(MIN + 2, 1.5),
                                     start=S, pairs=bias)[0]
            assert int(t[s]) == want, (s, cur[s], int(t[s]), want)
        return t

    setup(0, 77)
    model.prefill(prompt, px, slot=0)
    made = []
    for n in range(3):          # n = T - S + 0 .. 2: below the minimum, EOS is certain and held back
        made.append(int(step([0], {0: T + n}, {0: 77}, {0: n})[0]))
    assert EOSID not in made
    ids = torch.cat([prompt, torch.tensor(made, dtype=torch.int64)])
    L = int(ids.numel())
    # fork: slot 1 takes the KV at length L (two tokens below the minimum); resume: slot 2 holds the sequence from a plain prefill
    setup(1, 78)
    model.kv_fork(0, 1, L)
    model.prefill(ids, px, slot=1, reuse=True)
    model.set_sampling(slot=2, do_sample=False)
    model.prefill(ids, px, slot=2)
    setup(2, 79)
    model.resume_slot(2, ids, key)
    model.decode_batch_launch([2])
    t = model.decode_batch_wait()
    assert int(t[2]) == made[-1]                                      # the forced step samples nothing
    got = {1: [], 2: []}
    for n in range(3):
        t = step([1, 2], {1: L + n, 2: L + n}, {1: 78, 2: 79}, {1: n, 2: n})
        for s in (1, 2):
            got[s].append(int(t[s]))
    for s in (1, 2):          # two more held back, then EOS at exactly the minimum
        assert EOSID not in got[s][:2] and got[s][2] == EOSID, (s, got[s])
    # the reset: dtk_set_sampling_slot leaves the slot without values (an empty table, the plain draw)
    assert int(model.logit_bias_table(slot=1).count_nonzero()) == 1
    model.set_sampling(slot=1, do_sample=True, temperature=1.2, seed=78, bad_ids=[img])
    assert int(model.logit_bias_table(slot=1).count_nonzero()) == 0
    model.prefill(ids, px, slot=1)
    row = model.get_logits_slot(1)
    model.decode_batch_launch([1])
    t = model.decode_batch_wait()
    assert int(t[1]) == shape_oracle.draw(row, L, 1.2, 0, 1.0, 78, 0, bad=[img])[0] != EOSID
    del model
    gc.collect()
