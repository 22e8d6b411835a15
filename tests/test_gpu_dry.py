"""DRY on the MI355X: k_dry_scan over given histories (dtk_op_dry_scan) against tests/dry_oracle.py, the PN sampler instantiations with a
match table over given logits (dtk_op_sample_dry) in the three sampler families, the off path, one sequence end to end over the device's
own logits with the history read back, batched steps of the multi-vector and the MFMA family driven from the host and by both engines,
and the history across prefix reuse / dtk_kv_fork / dtk_resume_slot / dtk_score_packed."""
from __future__ import annotations

import ctypes as C
import gc
import threading

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from detikzify_amd.model.modeling import dry_struct
from oracle import sampling
from oracle.ops import rb
from tests import dry_oracle
from tests.helpers import TINY, sketch_image
from tests.test_gpu_penalty import _oracle_row, _raw_lse, _set
from tests.test_gpu_trunc import FAMILIES, _bigvocab

pytestmark = pytest.mark.gpu

BAD, BEGIN, SEED = [1], [2], 4711
DRAWS = 6
I64P = C.POINTER(C.c_int64)


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


def _scan(model, V, h, d, h2=None, n_max=4096):
    """dtk_op_dry_scan -> {id: M} of the whole table behind the last scan"""
    a1, p1 = _i64(h)
    a2, p2 = _i64(h2) if h2 is not None else (None, None)
    ids, ms = (C.c_int32 * n_max)(), (C.c_uint8 * n_max)()
    k = model.lib.dtk_op_dry_scan(model._ctx, V, p1, len(h), p2, len(h2) if h2 is not None else 0, C.byref(d), ids, ms, n_max)
    if k < 0:
        model._check(k, "dtk_op_dry_scan")
    assert k <= n_max
    return {int(ids[i]): int(ms[i]) for i in range(k)}


# ------------------------------------------------------------------------------------------ the scan alone
def test_op_dry_scan_matches_the_oracle(big):
    model, V = big, 40000
    a, b, c = 10, 11, 12
    Tmax = int(model.lib.dtk_max_positions(model._ctx))
    rng = np.random.default_rng(5)
    many = [t for j in range(320) for t in (7, 1000 + 97 * j)] + [7]          # 320 distinct continuations of one token
    cases = [("a b c a b", [a, b, c, a, b], 2, ()),
             ("allowed 3", [a, b, c, a, b], 3, ()),
             ("period 1", [5] * 10, 2, ()),
             ("period 1, cap", [5] * 100, 1, ()),
             ("period 3 x 30: cap", [a, b, c] * 30, 2, ()),
             ("period 3 x 21", [a, b, c] * 21, 2, ()),
             ("into position 0", [a, b, c, a, b, c], 2, ()),
             ("breaker last", [a, b, c, a, b], 1, (b,)),
             ("breaker next", [a, b, c, a, b], 1, (c,)),
             ("breaker inside", [9, a, b, c, 9, a, b], 1, (a,)),
             ("breaker outside", [9, a, b, c, 9, a, b], 1, (9, 3, 4)),
             ("n = 0", [], 1, ()), ("n = 1", [3], 1, ()), ("n = 2 same", [3, 3], 1, ()), ("n = 2", [3, 4], 1, ()),
             ("two continuations", [a, b, 1, 7, a, b, 2, 7, a, b], 2, ()),
             ("ids 0 and V - 1", [0, V - 1, 0, 0, V - 1, V - 1, 0, V - 1, 0], 1, ()),
             ("n = max_positions", rng.integers(0, 4, Tmax).tolist(), 2, ()),
             ("n = max_positions, breaker", rng.integers(0, 4, Tmax).tolist(), 2, (3,)),
             ("several strides", rng.integers(0, 3, 1500).tolist(), 3, ()),
             ("several strides, periodic", ([3, 1, 4, 1, 5, 9, 2, 6] * 200)[:1501], 2, ()),
             ("320 distinct ids", many, 1, ())]
    seen_cap = n_ids = 0
    for tag, h, al, brk in cases:
        d = dry_struct(0.8, 1.75, al, 0, brk)
        want = dry_oracle.penalised_ids(h, al, brk)
        got = _scan(model, V, h, d)
        assert got == want, (tag, got, want)
        seen_cap += 64 in got.values()
        n_ids = max(n_ids, len(got))
    assert seen_cap >= 3 and n_ids >= 300
    # two scans in a row on one state: nothing of the first survives (the second history penalises none of the first's ids)
    d = dry_struct(0.8, 1.75, 1, 0, ())
    first, second = many, [t for j in range(40) for t in (8, 35000 + 3 * j)] + [8]
    w1, w2 = dry_oracle.penalised_ids(first, 1), dry_oracle.penalised_ids(second, 1)
    assert len(w1) == 320 and len(w2) == 40 and not set(w1) & set(w2)
    assert _scan(model, V, first, d, second) == w2
    assert _scan(model, V, second, d, first) == w1
    assert _scan(model, V, first, d, [4]) == {}              # ... and a history that penalises nothing leaves an empty table
    assert _scan(model, V, [a, b, c] * 30, dry_struct(0.8, 1.75, 2, 0, ()), [a, b, c, a, b]) == {c: 2}
    # the ranges: DTK_ERR_ARG, nothing launched
    h, hp = _i64([1, 2, 1])
    ids, ms = (C.c_int32 * 4)(), (C.c_uint8 * 4)()
    for bad in (dry_struct(101.0, 1.75, 2, 0), dry_struct(float("nan"), 1.75, 2, 0), dry_struct(0.8, 0.5, 2, 0), dry_struct(0.8, 9.0, 2, 0),
                dry_struct(0.8, 1.75, 0, 0), dry_struct(0.8, 1.75, 65, 0), dry_struct(0.8, 1.75, 2, -1), dry_struct(0.8, 1.75, 2, 0, (V,))):
        assert model.lib.dtk_op_dry_scan(model._ctx, V, hp, 3, None, 0, C.byref(bad), ids, ms, 4) == -1
        assert model.lib.dtk_set_dry(model._ctx, C.byref(bad)) == -1
    over = dry_struct(0.8, 1.75, 2, 0)
    over.n_breakers = 17
    assert model.lib.dtk_set_dry(model._ctx, C.byref(over)) == -1
    bad_h, bp = _i64([1, V, 1])
    assert model.lib.dtk_op_dry_scan(model._ctx, V, bp, 3, None, 0, C.byref(dry_struct(0.8, 1.75, 2, 0)), ids, ms, 4) == -1


# ------------------------------------------------------------------------------------------ the samplers with a match table
def _history(ids3, ids2, ids1):
    """a history whose tail [Z, P, Q, R] matches with length 4 in front of ids3 (the Z in front matches too), 2 in front of ids2, 1 in
    front of ids1 (P, Q, R, Y, Z: small ids that carry no logit worth drawing); the oracle says what the lengths are"""
    P, Q, R, Y, Z = 31, 32, 33, 34, 35
    h = []
    for t in ids3:
        h += [Z, P, Q, R, t]
    for t in ids2:
        h += [Y, Q, R, t]
    for t in ids1:
        h += [Y, R, t]
    return h + [Z, P, Q, R]


def _rows(V):
    """(tag, logits, config, (m, b, a, breakers), history, (pp, fp, counted)).  The penalised ids sit where an index slip shows — 0 and
    V - 1, 8191 / 8192 (a slice boundary of the chain), the last 8-group of the row (ragged at 32 769: id 32 768 alone, the scalar branch
    of mb_load) — under match lengths 1, 2 and 4, each with a logit near the row's maximum so that its penalty moves the kept masses.
    Which kernels a row runs is the launchers' rule (tests/test_gpu_penalty.py::_rows): everything k_sample_fast at 32 000; at 32 769 and
    40 000 a sampling row with 0 < top_k < V runs k_sample, and a row with top_k = 0 or a greedy one the chain."""
    g = torch.Generator().manual_seed(V + 11)
    nk = V - 1 if V == 32769 else 0
    wide = lambda: rb(torch.randn(V, generator=g) * 4)
    last8 = (V - 1) // 8 * 8
    edge = [0, V - 1, 8191, 8192, last8, 8 * 1024 * 3 + 5]
    S = lambda T, k, p, mp=0.0, eps=0.0: dict(do_sample=True, temperature=T, top_k=k, top_p=p, min_p=mp, eps=eps)
    GREEDY = dict(do_sample=False, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, eps=0.0)
    h_edge = _history(edge[:2], edge[2:4], edge[4:])
    edges = wide().clone()
    edges[edge] = edges.max() - torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0, 1.25])
    moved = wide().clone()
    moved[V - 3] = moved.max() + 0.5           # the raw arg-max, matched with length 4: 0.8 * 1.75^2 = 2.45 off, greedy must leave it
    both = wide().clone()
    top = torch.topk(both, 6)[1].tolist()
    NONE = (0.0, 0.0, [])
    rows = [("edges", edges, S(1.0, nk, 1.0), (0.8, 1.75, 2, ()), h_edge, NONE),
            ("edges a1 + pair", edges, S(1.0, nk, 0.95), (0.5, 2.0, 1, ()), h_edge, (0.6, 0.4, [0, V - 1, V - 1, 8192, 77])),
            ("greedy moves", moved, GREEDY, (0.8, 1.75, 2, ()), _history([V - 3], [5], []), NONE),
            ("k50 p.9 min_p eps + pair", both, S(1.2, 50, 0.9, 0.1, 3e-4), (1.0, 1.75, 1, ()), _history(top[:1], top[1:2], top[3:4]),
             (0.6, 0.4, [top[0]] * 3 + [top[2]])),
            ("breaker", edges, S(1.0, nk, 1.0), (0.8, 1.75, 1, (32,)), h_edge, NONE)]
    if V > 32768:
        trunc = wide().clone()
        t6 = torch.topk(trunc, 6)[1].tolist()
        gtail = wide().clone()
        m = float(gtail.max())
        # raw: V - 1 wins.  z': V - 1 (the longest match) falls by more than 2 * 1.75 = 3.5, below m + 1.5, V - 2 (length 2) by 2 to
        # m + 2.0: id 100 (m + 2.4, not matched) wins only if BOTH entries were applied
        gtail[V - 1], gtail[V - 2], gtail[100] = m + 5.0, m + 4.0, m + 2.4
        rows += [("chain p.9 min_p eps", trunc, S(1.2, 0, 0.9, 0.1, 3e-4), (0.8, 1.75, 2, ()), _history(t6[:1] + [V - 1], t6[1:2] + [V - 2], t6[3:4]), NONE),
                 ("chain tail ids + pair", edges, S(1.0, 0, 0.95), (0.5, 2.0, 1, ()), h_edge, (0.6, 0.4, [V - 1] * 2 + [V - 2])),
                 ("chain greedy tail ids", gtail, GREEDY, (2.0, 1.75, 2, ()), _history([V - 1], [V - 2], []), NONE)]
    return rows


@pytest.mark.parametrize("V", list(FAMILIES), ids=[f"{v}-{k}" for v, k in FAMILIES.items()])
def test_op_sample_dry_matches_the_oracle(big, V):
    """every draw: the token is the oracle's over z'; the token, probs_out and sample_logprob are, bit for bit, what the same kernels give
    for the oracle's z' handed in as the row (dtk_op_sample_ext: everything behind the load sites is a function of z' alone); logprob is
    the bits of fp32(z[t] - L) over the RAW row, L read off dtk_op_sample_lp (tests/test_gpu_penalty.py::_raw_lse)"""
    model = big
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    tok, tok2, lp, lp2 = C.c_int64(), C.c_int64(), (C.c_float * 2)(), (C.c_float * 2)()
    probs, probs2 = np.empty(V, dtype=np.float32), np.empty(V, dtype=np.float32)
    n_rows = 0
    for tag, logits, cfg, (m, b, a, brk), hist, (pp, fp, counted) in _rows(V):
        n_rows += 1
        lb = logits.numpy().copy()
        _, hp = _h = _i64(hist)
        _, cp = _c = _i64(counted)
        d = dry_struct(m, b, a, 0, brk)
        _set(model, cfg)
        x = _lib.DtkSamplingExt(min_p=cfg["min_p"], epsilon_cutoff=cfg["eps"])
        pens = dry_oracle.penalised_ids(hist, a, brk)
        zp = dry_oracle.both(logits, counted, pp, fp, hist, m, b, a, brk)
        touched = sorted(set(pens) | set(counted))
        untouched = torch.ones(V, dtype=torch.bool); untouched[touched] = False
        assert len(pens) >= 2 and torch.equal(zp[untouched], logits[untouched]) and bool((zp[touched] != logits[touched]).all()), (V, tag)
        zb = zp.numpy().copy()
        L = _raw_lse(model, lb, logits, V, 8)
        assert L is not None, (V, tag, "no draw of dtk_op_sample_lp gives the raw logsumexp exactly")
        lp_bits = lambda t: bytes(C.c_float(float(np.float32(np.float32(float(logits[t])) - L))))
        call = lambda n, t, pr, l: model._check(model.lib.dtk_op_sample_dry(model._ctx, ptr(lb), V, n, C.byref(t), pr, l, C.byref(x), pp, fp, cp,
                                                                            len(counted), hp, len(hist), C.byref(d)), "dtk_op_sample_dry")
        ref_call = lambda n: model._check(model.lib.dtk_op_sample_ext(model._ctx, ptr(zb), V, n, C.byref(tok2), ptr(probs2), lp2, C.byref(x)),
                                          "dtk_op_sample_ext")
        if not cfg["do_sample"]:
            want, raw = sampling.greedy(zp, BAD, BEGIN, True), sampling.greedy(logits, BAD, BEGIN, True)
            assert want != raw, (V, tag)               # the row shows something: the penalty moves the arg-max
            call(0, tok, ptr(probs), lp)
            assert tok.value == want and probs[want] == 1.0 and int((probs != 0).sum()) == 1, (V, tag, tok.value, want)
            assert bytes(C.c_float(lp[0])) == lp_bits(want) and lp[1] == 0.0, (V, tag, lp[0], lp[1])
            call(0, tok, None, None)
            assert tok.value == want
            continue
        ref = {first: _oracle_row(zp, cfg, first) for first in (True, False)}
        assert not torch.equal(ref[False][0], _oracle_row(logits, cfg, False)[0]), (V, tag, "the penalty does not move the kept masses")
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
    assert n_rows == (5 if V <= 32768 else 8)


@pytest.mark.parametrize("V", list(FAMILIES), ids=[f"{v}-{k}" for v, k in FAMILIES.items()])
def test_off_means_off_at_op_level(big, V):
    """multiplier 0 with a history full of matches: the token, the probabilities and both log-probabilities of dtk_op_sample_ext, bit
    for bit"""
    model = big
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    logits = rb(torch.randn(V, generator=torch.Generator().manual_seed(V + 1)) * 4)
    lb = logits.numpy().copy()
    _, hp = _h = _i64(_history([0, V - 1, int(logits.argmax())], [8191], [8192]))
    d = dry_struct(0.0, 1.75, 1, 0)
    tok, tok2, lp, lp2 = C.c_int64(), C.c_int64(), (C.c_float * 2)(), (C.c_float * 2)()
    p1, p2 = np.empty(V, dtype=np.float32), np.empty(V, dtype=np.float32)
    for T, k, p, mp, eps in ((0.8, V - 1 if V == 32769 else 0, 0.95, 0.0, 0.0), (1.3, 50, 1.0, 0.1, 3e-4)):
        model.set_sampling(do_sample=True, temperature=T, top_p=p, top_k=k, seed=SEED, bad_ids=BAD, begin_suppress_ids=BEGIN)
        x = _lib.DtkSamplingExt(min_p=mp, epsilon_cutoff=eps)
        for n in range(DRAWS):
            model._check(model.lib.dtk_op_sample_dry(model._ctx, ptr(lb), V, n, C.byref(tok), ptr(p1), lp, C.byref(x), 0.0, 0.0, None, 0,
                                                     hp, len(_h[0]), C.byref(d)), "dtk_op_sample_dry")
            model._check(model.lib.dtk_op_sample_ext(model._ctx, ptr(lb), V, n, C.byref(tok2), ptr(p2), lp2, C.byref(x)), "dtk_op_sample_ext")
            assert tok.value == tok2.value and p1.tobytes() == p2.tobytes() and bytes(lp) == bytes(lp2), (V, T, k, n)


# ------------------------------------------------------------------------------------------ one sequence, end to end
# The toy models' logits are flat: at temperature 1 a sampled run never repeats itself and DRY would have nothing to change.  The
# in-step tests sample at TEMP = 0.1, where the toys loop as a real model does (the sampled path of every kernel still runs: masses,
# histograms, the draw), and assert that DRY changed the run, not only that the device agrees with the oracle.
TEMP = 0.1
M_, B_, A_ = 3.0, 1.75, 1
TAIL = [77, 30, 9, 77, 30, 9, 77, 30]


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


@pytest.mark.parametrize("name", ["detikzify-tiny", "tiny-v2-40000"])
def test_generate_is_the_oracle_draw_over_the_device_logits(name):
    """48 tokens of generate(dry_multiplier=...) == the same steps driven by hand, each of which is the oracle's draw over the row the
    device sampled from under the history so far (k_sample_fast on the toy vocabulary, the multi-block chain at 40 000), and NOT the
    plain run: on some step the draw over z' is another token than the draw over the raw row.  The history is read back on the way;
    then the same with top_logprobs on: the records stay those of the raw row while the arg-max moves"""
    model, ids, px, img, S = _single(name)
    T = int(ids.numel())
    state = lambda: int(model.lib.dtk_dry_state_bytes(model._ctx))
    assert state() == 0 and model.dry_history().numel() == 0
    GEN = dict(input_ids=ids[None], pixel_values=px, max_new_tokens=48, eos_token_id=-1, bad_words_ids=[[img]], seed=31, do_sample=True,
               temperature=TEMP, top_k=0)
    plain = model.generate(**GEN)[0, T:].tolist()
    assert model.generate(dry_multiplier=0.0, dry_base=3.0, dry_start=0, **GEN)[0, T:].tolist() == plain
    assert state() == 0                                       # a context that never had a multiplier has allocated nothing
    new = model.generate(dry_multiplier=M_, dry_base=B_, dry_allowed_length=A_, dry_start=S, **GEN)[0, T:].tolist()
    assert len(new) == 48 and new != plain                    # DRY changed the run
    assert state() > 0
    assert model.generate(**GEN)[0, T:].tolist() == plain     # ... and a later plain call is the plain run again
    assert model.dry_history().numel() == 0                   # (it reset the record: an empty history)
    model.set_sampling(do_sample=True, temperature=TEMP, seed=31, bad_ids=[img])
    model.set_dry(M_, B_, A_, S)
    model.prefill(ids, px)
    assert model.dry_history().tolist() == TAIL
    made, moved = [], 0
    for n in range(48):
        row = model.get_logits()
        model.decode_launch()
        if n == 5:            # refused while a step is unread (DTK_ERR_STATE), and nothing changes
            assert model.lib.dtk_set_dry(model._ctx, C.byref(dry_struct(1.0, 2.0, 2, 0))) == -3
        tok = model.decode_wait()
        hist = TAIL + made
        want, _, _ = dry_oracle.draw(row, hist, M_, B_, A_, (), TEMP, 0, 1.0, 31, n, bad=[img])
        raw, _, _ = dry_oracle.draw(row, hist, 0.0, B_, A_, (), TEMP, 0, 1.0, 31, n, bad=[img])
        assert tok == want == new[n], (name, n, tok, want, new[n])
        moved += want != raw                                  # the device's token is the draw over z', and the raw row's is another
        made.append(tok)
        if n in (0, 17, 47):
            assert model.dry_history().tolist() == TAIL + made, n
    print(f"{name}: 48 tokens exact; the draw over z' is not the raw row's on {moved} steps; {sum(a != b for a, b in zip(new, plain))} of 48 differ from the plain run")
    assert moved >= 1
    # the values change on a live sequence: the history is rebuilt from its ids under the new start (here: the whole text)
    model.set_dry(M_, B_, A_, 0, breakers=(5,))
    assert model.dry_history().tolist() == ids.tolist() + made
    model.set_dry(M_, B_, A_, T + 50)                         # a start the sequence has not reached: nothing is kept, also of the next token
    assert model.dry_history().numel() == 0
    model.decode_launch(); extra = model.decode_wait()
    assert model.dry_history().numel() == 0
    model.set_dry(M_, B_, A_, T + 48)
    assert model.dry_history().tolist() == [extra]
    # top_logprobs: the records and the logprob are over the raw row, the token over z'
    model.set_sampling(do_sample=False, bad_ids=[img])
    model.set_dry(100.0, 1.0, 1, S)
    model.enable_top_logprobs(3)
    model.prefill(ids, px)
    made, moved = [], 0
    for n in range(8):
        row = model.get_logits()
        model.decode_launch()
        tok, lp, _, top_ids, top_lps = model.decode_wait(top=True)
        hist = TAIL + made
        assert tok == dry_oracle.greedy(row, hist, 100.0, 1.0, 1, bad=[img])
        ref = torch.log_softmax(row.double(), 0)
        order = sorted(range(row.numel()), key=lambda i: (-float(row[i]), i))[:3]
        assert list(top_ids) == order and np.allclose(list(top_lps), [float(ref[i]) for i in order], atol=1e-4), (n, top_ids, order)
        assert abs(lp - float(ref[tok])) < 1e-4
        moved += tok != sampling.greedy(row, [img], [], n == 0)
        made.append(tok)
    print(f"{name}: top_logprobs raw on 8 greedy steps; DRY moved the arg-max on {moved}")
    assert moved >= 1                                          # the token is z''s arg-max where the records' first id is the raw one
    # dtk_score_packed leaves no sequence: an empty history
    model.set_sampling(do_sample=False, bad_ids=[img])
    model.set_dry(M_, B_, A_, 0)
    model.prefill(ids, px)
    assert model.dry_history().tolist() == ids.tolist()
    model.score_candidates(ids, [torch.tensor([77, 30, 9])], px, reuse=False)
    assert model.dry_history().numel() == 0
    del model
    gc.collect()


# ------------------------------------------------------------------------------------------ batched steps
# slot s: (multiplier, base, allowed_length, start (None: the end of the image prompt), breakers)
SETS = [(3.0, 1.75, 1, None, ()), (0.0, 1.75, 2, None, ()), (0.8, 2.0, 1, 0, ()), (5.0, 1.0, 1, None, (41,))]
STEPS = 12


def _prompts(proc, n):
    enc = proc(images=sketch_image(5, 96), return_tensors="pt")
    base, px = enc.input_ids[0], enc.pixel_values
    tails = [[20 + s, 41 + s, 20 + s, 41 + s, 60, 20 + s] for s in range(n)]
    return [torch.cat([base, torch.tensor(t, dtype=torch.int64)]) for t in tails], px, int(base.numel())


def _start(S, s):
    return S if SETS[s][3] is None else SETS[s][3]


def _drive(model, prompts, px, S, slots, check):
    """STEPS batched steps of `slots` driven from the host; check: every token against the oracle's draw over the slot's own logits"""
    for s in slots:
        m, b, a, _, brk = SETS[s]
        model.set_sampling(slot=s, do_sample=True, temperature=TEMP, seed=900 + s, bad_ids=[TINY.image_token_id])
        if m:
            model.set_dry(m, b, a, _start(S, s), brk, slot=s)
        model.prefill(prompts[s], px, slot=s)
    toks = {s: [] for s in slots}
    for n in range(STEPS):
        rows = {s: model.get_logits_slot(s) for s in slots} if check else {}
        model.decode_batch_launch(slots)
        t = model.decode_batch_wait()
        for s in slots:
            if check:
                m, b, a, _, brk = SETS[s]
                hist = prompts[s].tolist()[_start(S, s):] + toks[s]
                want, _, _ = dry_oracle.draw(rows[s], hist, m, b, a, brk, TEMP, 0, 1.0, 900 + s, n, bad=[TINY.image_token_id])
                assert t[s] == want, (s, n, t[s], want)
            toks[s].append(int(t[s]))
    if check:
        for s in slots:
            hist = prompts[s].tolist()[_start(S, s):] + toks[s] if SETS[s][0] else []
            assert model.dry_history(slot=s).tolist() == hist, s
    return toks


@pytest.fixture(scope="module", params=[5, 17], ids=["mv-4", "mfma-16"])
def batched(request):
    """detikzify-tiny with 5 slots (slots 0..3 decode with the multi-vector kernels) and with 17 (one MFMA column tile)"""
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny", synthetic=1234, batch_slots=request.param)
    assert model.max_decode_slots() == (4 if request.param == 5 else 16)
    prompts, px, S = _prompts(proc, 4)
    hand = _drive(model, prompts, px, S, [0, 1, 2, 3], check=True)       # (before anything switches the log-probabilities on)
    yield model, prompts, px, S, hand
    del model
    gc.collect()


def test_slots_with_their_own_values_are_exact_and_as_alone(batched):
    model, prompts, px, S, hand = batched
    for s in range(4):
        assert _drive(model, prompts, px, S, [s], check=False)[s] == hand[s], s
    # the values matter: slot 1 (off) is the plain sampler's sequence, and some other slot's is not what it would be without DRY
    plain = {}
    for s in range(4):
        model.set_sampling(slot=s, do_sample=True, temperature=TEMP, seed=900 + s, bad_ids=[TINY.image_token_id])
        model.prefill(prompts[s], px, slot=s)
    for n in range(STEPS):
        model.decode_batch_launch([0, 1, 2, 3])
        t = model.decode_batch_wait()
        for s in range(4):
            plain.setdefault(s, []).append(int(t[s]))
    assert plain[1] == hand[1]
    assert all(model.dry_history(slot=s).numel() == 0 for s in range(4))
    print("slots whose run DRY changed:", [s for s in (0, 2, 3) if plain[s] != hand[s]])
    assert plain[0] != hand[0] and plain[2] != hand[2]          # each slot's own table was applied in the step (slot stride, graph)
    # DRY on slot 1 only: slot 0 draws what it draws alone
    for s in (0, 1):
        model.set_sampling(slot=s, do_sample=True, temperature=TEMP, seed=900 + s, bad_ids=[TINY.image_token_id])
        if s == 1:
            model.set_dry(3.0, 1.75, 1, S, slot=1)
        model.prefill(prompts[s], px, slot=s)
    got0 = []
    for n in range(STEPS):
        model.decode_batch_launch([0, 1])
        got0.append(int(model.decode_batch_wait()[0]))
    assert got0 == plain[0]


@pytest.mark.parametrize("engine", ["native", "python"])
def test_engines_carry_the_values_with_the_joins(batched, engine):
    """four sequences with their own values through either engine: the tokens of the same slots driven by hand, which the fixture checked
    against the oracle; a later join without values inherits nothing"""
    from detikzify_amd.infer.batching import BatchEngine
    from detikzify_amd.infer.engine import NativeBatchEngine
    model, prompts, px, S, hand = batched
    eng = (NativeBatchEngine if engine == "native" else BatchEngine)(model, max_batch=4, share_prefix=False, resume_in_place=False)
    got, errs = {}, []
    common = dict(pixel_values=px, max_new_tokens=STEPS, eos_token_id=-1, bad_words_ids=[[TINY.image_token_id]], do_sample=True,
                  temperature=TEMP, top_k=0)
    dry = lambda s: dict(dry_multiplier=SETS[s][0], dry_base=SETS[s][1], dry_allowed_length=SETS[s][2], dry_start=_start(S, s),
                         dry_sequence_breakers=list(SETS[s][4]))

    def run(s):
        try:
            got[s] = model.generate(input_ids=prompts[s][None], seed=900 + s, **dry(s), **common)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    try:
        ths = [threading.Thread(target=run, args=(s,)) for s in range(4)]
        [t.start() for t in ths]
        [t.join(timeout=120) for t in ths]
        assert not any(t.is_alive() for t in ths) and not errs, errs[:1]
        again = model.generate(input_ids=prompts[0][None], seed=900, **common)
        again_dry = model.generate(input_ids=prompts[0][None], seed=900, **dry(0), **common)
    finally:
        eng.close()
    T = [p.numel() for p in prompts]
    for s in range(4):
        assert got[s][0, T[s]:].tolist() == hand[s], (engine, s)
    assert again_dry[0, T[0]:].tolist() == hand[0]
    model.set_sampling(slot=0, do_sample=True, temperature=TEMP, seed=900, bad_ids=[TINY.image_token_id])
    model.prefill(prompts[0], px, slot=0)
    ref = []
    for n in range(STEPS):
        model.decode_batch_launch([0])
        ref.append(int(model.decode_batch_wait()[0]))
    assert again[0, T[0]:].tolist() == ref and ref != hand[0]      # the join without values is the plain run, which DRY's is not


# ------------------------------------------------------------------------------------------ the chain, batched
def test_two_slots_of_the_chain_with_their_own_values():
    """the 40 000-token toy with slots: the multi-block chain with a slot offset on the match table (sample_bind_slot), k_dry_scan with one block
    per slot in front of it and the trailing kernel behind it, 10 steps of two slots under different values.  Every token is the
    oracle's draw over z' of the slot's own row, and in each slot some step's draw is not the raw row's"""
    model = _bigvocab(slots=3)
    cfg = model.config
    img, P = cfg.image_token_id, cfg.num_patches
    px = torch.zeros(1, 3, cfg.vit_image, cfg.vit_image)
    prompts = [torch.tensor([img] * P + TAIL), torch.tensor([img] * P + [8192, 39999, 8192, 39999, 8192])]
    vals = [(3.0, 1.75, 1, P, ()), (5.0, 1.75, 2, P, ())]
    for s in (0, 1):
        model.set_sampling(slot=s, do_sample=True, temperature=TEMP, top_p=0.95, seed=500 + s, bad_ids=[img])
        model.set_dry(*vals[s], slot=s)
        model.prefill(prompts[s], px, slot=s)
    toks, moved = {0: [], 1: []}, {0: 0, 1: 0}
    for n in range(10):
        rows = {s: model.get_logits_slot(s) for s in (0, 1)}
        model.decode_batch_launch([0, 1])
        t = model.decode_batch_wait()
        for s in (0, 1):
            m, b, a, st, brk = vals[s]
            hist = prompts[s].tolist()[st:] + toks[s]
            want, _, _ = dry_oracle.draw(rows[s], hist, m, b, a, brk, TEMP, 0, 0.95, 500 + s, n, bad=[img])
            raw, _, _ = dry_oracle.draw(rows[s], hist, 0.0, b, a, brk, TEMP, 0, 0.95, 500 + s, n, bad=[img])
            assert int(t[s]) == want, (s, n, int(t[s]), want)
            moved[s] += want != raw
            toks[s].append(int(t[s]))
    print("chain, 2 slots: steps on which the draw over z' is not the raw row's:", moved)
    assert moved[0] >= 1 and moved[1] >= 1
    for s in (0, 1):
        assert model.dry_history(slot=s).tolist() == prompts[s].tolist()[vals[s][3]:] + toks[s], s
    del model
    gc.collect()


# ------------------------------------------------------------------------------------------ the history follows the sequence
def test_the_history_follows_fork_resume_and_prefix_reuse():
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny", synthetic=1234, batch_slots=5)
    prompts, px, S = _prompts(proc, 1)
    prompt, img = prompts[0], TINY.image_token_id
    T = int(prompt.numel())
    key = model.image_key(px)

    def setup(s, seed):
        model.set_sampling(slot=s, do_sample=True, temperature=1.2, seed=seed, bad_ids=[img])
        model.set_dry(M_, B_, A_, S, slot=s)

    setup(0, 77)
    model.prefill(prompt, px, slot=0)
    text = prompt.tolist()[S:]
    assert model.dry_history(slot=0).tolist() == text
    made = []
    for n in range(8):
        model.decode_batch_launch([0])
        made.append(int(model.decode_batch_wait()[0]))
    ids = torch.cat([prompt, torch.tensor(made, dtype=torch.int64)])
    assert model.dry_history(slot=0).tolist() == text + made
    # fork: slot 1 takes the history with the KV; the prefill of the last token on top rebuilds the same one
    setup(1, 78)
    model.kv_fork(0, 1, int(ids.numel()))
    assert model.dry_history(slot=1).tolist() == text + made
    model.prefill(ids, px, slot=1, reuse=True)
    assert model.dry_history(slot=1).tolist() == text + made
    # resume: slot 2 holds the sequence from an earlier (plain) prefill; the forced last token is in the history once, by the rebuild
    model.set_sampling(slot=2, do_sample=False)
    model.prefill(ids, px, slot=2)
    assert model.dry_history(slot=2).numel() == 0
    setup(2, 79)
    model.resume_slot(2, ids, key)
    assert model.dry_history(slot=2).tolist() == text + made
    model.set_dry(M_, B_, A_, S, slot=2)                          # set again before the forced step: the forced id is still there
    assert model.dry_history(slot=2).tolist() == text + made
    model.decode_batch_launch([1, 2])
    t = model.decode_batch_wait()
    assert int(t[2]) == made[-1]                                  # the forced token
    assert model.dry_history(slot=2).tolist() == text + made      # ... is not appended a second time
    assert model.dry_history(slot=1).tolist() == text + made + [int(t[1])]
    rows = {2: model.get_logits_slot(2)}
    model.decode_batch_launch([2])
    t2 = model.decode_batch_wait()
    want2, _, _ = dry_oracle.draw(rows[2], text + made, M_, B_, A_, (), 1.2, 0, 1.0, 79, 0, bad=[img])
    assert int(t2[2]) == want2
    assert model.dry_history(slot=2).tolist() == text + made + [want2]
    # a DTK_PREFILL_REUSE_PREFIX prefill of a shorter prompt drops the cut tokens
    model.prefill(ids[:T + 3], px, slot=0, reuse=True)
    assert model.dry_history(slot=0).tolist() == text + made[:3]
    del model
    gc.collect()
