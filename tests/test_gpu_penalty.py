"""presence_penalty / frequency_penalty on the MI355X: the PN instantiations of the three sampler families over given logits
(dtk_op_sample_pen) against tests/penalty_oracle.py, the off path against dtk_op_sample_ext, one sequence end to end over the device's
own logits with the count table read back, greedy, batched steps of the multi-vector and the MFMA family driven from the host and by
both engines, and the table across dtk_kv_fork / dtk_resume_slot / a DTK_PREFILL_REUSE_PREFIX prefill."""
from __future__ import annotations

import ctypes as C
import gc
import math
import threading
from collections import Counter

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from oracle import sampling
from oracle.ops import rb
from tests import penalty_oracle, trunc_oracle
from tests.helpers import TINY, sketch_image
from tests.test_gpu_trunc import FAMILIES, _bigvocab

pytestmark = pytest.mark.gpu

BAD, BEGIN, SEED = [1], [2], 4711
DRAWS = 8


@pytest.fixture(scope="module")
def big():
    m = _bigvocab()
    m.enable_logprobs()
    yield m
    del m
    gc.collect()


def _rows(V):
    """(tag, logits, config, pp, fp, counted ids, raw arg-max of a greedy row).  The counted ids sit where an index slip shows — ids 0 and
    V - 1, 8191 / 8192 (a slice boundary of the chain), the last 8-group of the row (ragged at 32 769: id 32 768 alone) — with counts of 1
    and of 7, and each carries a logit near the row's maximum, so that its penalty moves the kept masses.

    Which kernels a row runs is the launchers' rule (FAMILIES): at 32 000 everything is k_sample_fast.  At 32 769 and 40 000 a sampling row
    with 0 < top_k < V runs k_sample — the first four rows at 32 769 (top_k = V - 1 or 50), and the "k50" row at 40 000, which therefore
    does NOT run the chain — and a row with top_k = 0, or a greedy one, runs the chain.  The "chain" rows (V > 32 768 only) carry top_k = 0
    so that the chain sees what the issue names for every family: top-p + min-p + epsilon (k_smb_kept<true>, k_smb_trunc, k_smb_draw<*, true>
    under PN), and counted ids V - 1 and V - 2 under sampling and under greedy — at 32 769 id 32 768 is the row's ragged tail, the scalar
    branch of mb_load, and 32 767 the last element of the last full group."""
    g = torch.Generator().manual_seed(V + 7)
    nk = V - 1 if V == 32769 else 0
    wide = lambda: rb(torch.randn(V, generator=g) * 4)
    last8 = (V - 1) // 8 * 8
    edge_ids = [0, V - 1, 8191, 8192, last8, 8 * 1024 * 3 + 5]
    edges = wide().clone()
    edges[edge_ids] = edges.max() - torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0, 1.25])
    edge_counted = [0, V - 1, 8191] + [8192] * 7 + [last8] * 2 + [edge_ids[5]] * 3
    moved = wide().clone()
    moved[V - 3] = moved.max() + 0.5           # the raw arg-max, counted 7 times: greedy must leave it
    both = wide().clone()
    top = torch.topk(both, 6)[1].tolist()
    neg = wide().clone()
    mid = torch.topk(neg, 40)[1].tolist()[20:26]
    S = lambda T, k, p, mp=0.0, eps=0.0: dict(do_sample=True, temperature=T, top_k=k, top_p=p, min_p=mp, eps=eps)
    GREEDY = dict(do_sample=False, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, eps=0.0)
    rows = [("edges c1 c7", edges, S(1.0, nk, 1.0), 0.6, 0.4, edge_counted, None),
            ("greedy moves", moved, GREEDY, 0.6, 0.4, [V - 3] * 7 + [5], V - 3),
            ("k50 p.9 min_p eps", both, S(1.2, 50, 0.9, 0.1, 3e-4), 0.6, 0.4, [top[0]] * 7 + [top[1]] + [top[3]] * 2, None),
            ("negative", neg, S(1.0, nk, 0.95), -0.5, -0.25, mid + mid[:2] * 3, None)]
    if V > 32768:
        trunc = wide().clone()
        t6 = torch.topk(trunc, 6)[1].tolist()
        tail = wide().clone()
        m = float(tail.max())
        tail[V - 1], tail[V - 2] = m + 1.0, m + 0.5
        gtail = wide().clone()
        m = float(gtail.max())
        # raw: V - 1 wins.  z': V - 1 falls by .6 + .4 * 7 = 3.4 to m + 1.6, V - 2 by .6 + .4 * 3 = 1.8 to m + 2.2: id 100 (m + 2.4, not
        # counted) wins only if BOTH counts were applied
        gtail[V - 1], gtail[V - 2], gtail[100] = m + 5.0, m + 4.0, m + 2.4
        rows += [("chain p.9 min_p eps", trunc, S(1.2, 0, 0.9, 0.1, 3e-4), 0.6, 0.4, [t6[0]] * 7 + [t6[1]] + [t6[3]] * 2 + [V - 1, V - 2], None),
                 ("chain tail ids", tail, S(1.0, 0, 0.95), 0.6, 0.4, [V - 1] * 7 + [V - 2], None),
                 ("chain greedy tail ids", gtail, GREEDY, 0.6, 0.4, [V - 1] * 7 + [V - 2] * 3, V - 1)]
    return rows


def _oracle_row(z, cfg, first):
    """(kept masses, total, running sum) of a row under cfg: the same for every draw counter with the same `first`"""
    _, q, keep = trunc_oracle.kept_set(z, cfg["temperature"], cfg["top_k"], cfg["top_p"], cfg["min_p"], cfg["eps"], BAD, BEGIN, first)
    qk = torch.where(keep, q, torch.zeros_like(q))
    return qk, int(qk.sum()), torch.cumsum(qk, 0)


def _set(model, cfg, seed=SEED):
    if cfg["do_sample"]:
        model.set_sampling(do_sample=True, temperature=cfg["temperature"], top_p=cfg["top_p"], top_k=cfg["top_k"], seed=seed, bad_ids=BAD,
                           begin_suppress_ids=BEGIN)
    else:
        model.set_sampling(do_sample=False, bad_ids=BAD, begin_suppress_ids=BEGIN)


def _raw_lse(model, lb, logits, V, draws):
    """the fp32 logsumexp of the RAW row as the LP kernels form it, read off dtk_op_sample_lp: logprob = fp32(z[t] - L), and the
    subtraction is exact (Sterbenz) whenever L / 2 <= z[t] <= 2 L, so L = z[t] - logprob exactly for such a token.  L does not depend on
    the token, which makes every later logprob of the row checkable to the bit: fp32(z[t] - L)"""
    tok, lp = C.c_int64(), (C.c_float * 2)()
    for n in range(draws):
        model._check(model.lib.dtk_op_sample_lp(model._ctx, lb.ctypes.data_as(C.c_void_p), V, n, C.byref(tok), None, lp), "dtk_op_sample_lp")
        zt = float(logits[tok.value])
        L = zt - float(lp[0])              # two fp32 values: exact in double
        if L > 0 and L / 2 <= zt <= 2 * L and float(np.float32(L)) == L:
            return np.float32(L)
    return None


@pytest.mark.parametrize("V", list(FAMILIES), ids=[f"{v}-{k}" for v, k in FAMILIES.items()])
def test_op_sample_pen_matches_the_oracle(big, V):
    """token and kept set exact, probabilities to 1e-5 relative, sample_logprob to 1e-6 relative (the bars of
    tests/test_gpu_trunc.py::test_op_sample_ext_matches_the_oracle); logprob, on EVERY draw, the bits of fp32(z[t] - L) over the raw row,
    L read off dtk_op_sample_lp (_raw_lse), and the bits dtk_op_sample_lp itself gives where it draws the same token.  Which rows run
    which kernels: _rows."""
    model = big
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    tok, tok2, lp, lp2 = C.c_int64(), C.c_int64(), (C.c_float * 2)(), (C.c_float * 2)()
    probs = np.empty(V, dtype=np.float32)
    same_tok = n_rows = 0
    for tag, logits, cfg, pp, fp, counted, raw_argmax in _rows(V):
        n_rows += 1
        lb = logits.numpy().copy()
        ids = np.asarray(counted, dtype=np.int64)
        idp = ids.ctypes.data_as(C.POINTER(C.c_int64))
        _set(model, cfg)
        x = _lib.DtkSamplingExt(min_p=cfg["min_p"], epsilon_cutoff=cfg["eps"])
        zp = penalty_oracle.penalise(logits, counted, pp, fp)
        untouched = torch.ones(V, dtype=torch.bool); untouched[list(set(counted))] = False
        assert torch.equal(zp[untouched], logits[untouched]) and bool((zp[~untouched] != logits[~untouched]).all())
        L = _raw_lse(model, lb, logits, V, DRAWS)
        assert L is not None, (V, tag, "no draw of dtk_op_sample_lp gives the raw logsumexp exactly")
        lp_bits = lambda t: bytes(C.c_float(float(np.float32(np.float32(float(logits[t])) - L))))
        call = lambda n, t, pr, l: model._check(model.lib.dtk_op_sample_pen(model._ctx, ptr(lb), V, n, C.byref(t), pr, l, C.byref(x),
                                                                            pp, fp, idp, len(counted)), "dtk_op_sample_pen")
        if not cfg["do_sample"]:
            want, raw = sampling.greedy(zp, BAD, BEGIN, True), sampling.greedy(logits, BAD, BEGIN, True)
            assert want != raw == raw_argmax, (V, tag)               # the row shows something: the penalty moves the arg-max
            call(0, tok, ptr(probs), lp)
            assert tok.value == want and probs[want] == 1.0 and int((probs != 0).sum()) == 1, (V, tag, tok.value, want)
            call(0, tok2, None, None)
            assert tok2.value == want
            assert bytes(C.c_float(lp[0])) == lp_bits(want) and lp[1] == 0.0, (V, tag, lp[0], lp[1])
            continue
        ref = {first: _oracle_row(zp, cfg, first) for first in (True, False)}
        plain = _oracle_row(logits, cfg, False)
        assert not torch.equal(ref[False][0], plain[0]), (V, tag, "the penalty does not move the kept masses: the row shows nothing")
        for n in range(DRAWS):
            qk, total, run = ref[n == 0]
            target = (total * sampling.rand32(SEED, n)) >> 32
            want = int(torch.searchsorted(run, torch.tensor(target, dtype=torch.int64), right=True))
            call(n, tok, ptr(probs), lp)
            t = tok.value
            assert t == want, (V, tag, n, t, want)
            rp = (qk.double() / float(total)).float().numpy()
            assert int(((probs > 0) ^ (rp > 0)).sum()) == 0, (V, tag, n, "kept sets differ")
            assert np.allclose(probs, rp, rtol=1e-5, atol=1e-9), (V, tag, n)
            slp = math.log(int(qk[t]) / total)
            assert abs(lp[1] - slp) <= 1e-6 * abs(slp) if slp != 0.0 else lp[1] == 0.0, (V, tag, n, lp[1], slp)
            assert bytes(C.c_float(lp[0])) == lp_bits(t), (V, tag, n, lp[0])
            if n % 4 == 0:      # the kernels without the log-probability code: the same token
                call(n, tok2, None, None)
                assert tok2.value == t, (V, tag, n)
            model._check(model.lib.dtk_op_sample_lp(model._ctx, ptr(lb), V, n, C.byref(tok2), None, lp2), "dtk_op_sample_lp")
            if tok2.value == t:
                same_tok += 1
                assert bytes(C.c_float(lp[0])) == bytes(C.c_float(lp2[0])), (V, tag, n)
    print(f"op_sample_pen V={V} ({FAMILIES[V]}): {n_rows} rows exact, logprob bits on every draw; {same_tok} draws chose dtk_op_sample_lp's token")
    assert n_rows == (4 if V <= 32768 else 7)
    # the ranges: DTK_ERR_ARG, nothing launched
    lb = np.zeros(8, dtype=np.float32)
    one = np.asarray([3], dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    for pp, fp in ((2.5, 0.0), (0.0, -2.5), (float("nan"), 0.0), (0.0, float("inf"))):
        assert model.lib.dtk_op_sample_pen(model._ctx, ptr(lb), 8, 0, C.byref(tok), None, None, None, pp, fp, one, 1) == -1
        assert model.lib.dtk_set_penalties(model._ctx, pp, fp, 0) == -1
    assert model.lib.dtk_set_penalties(model._ctx, 0.5, 0.5, -1) == -1
    bad_id = np.asarray([8], dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    assert model.lib.dtk_op_sample_pen(model._ctx, ptr(lb), 8, 0, C.byref(tok), None, None, None, 0.5, 0.5, bad_id, 1) == -1


@pytest.mark.parametrize("V", list(FAMILIES), ids=[f"{v}-{k}" for v, k in FAMILIES.items()])
def test_off_means_off(big, V):
    """0 / 0 with a non-empty id list: the token, the probabilities and both log-probabilities of dtk_op_sample_ext, bit for bit"""
    model = big
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    logits = rb(torch.randn(V, generator=torch.Generator().manual_seed(V + 1)) * 4)
    lb = logits.numpy().copy()
    ids = np.asarray([0, V - 1, 8191, 8192, 8192, int(logits.argmax())] * 3, dtype=np.int64)
    idp = ids.ctypes.data_as(C.POINTER(C.c_int64))
    tok, tok2, lp, lp2 = C.c_int64(), C.c_int64(), (C.c_float * 2)(), (C.c_float * 2)()
    p1, p2 = np.empty(V, dtype=np.float32), np.empty(V, dtype=np.float32)
    for T, k, p, mp, eps in ((0.8, V - 1 if V == 32769 else 0, 0.95, 0.0, 0.0), (1.3, 50, 1.0, 0.1, 3e-4)):
        model.set_sampling(do_sample=True, temperature=T, top_p=p, top_k=k, seed=SEED, bad_ids=BAD, begin_suppress_ids=BEGIN)
        x = _lib.DtkSamplingExt(min_p=mp, epsilon_cutoff=eps)
        for n in range(DRAWS):
            model._check(model.lib.dtk_op_sample_pen(model._ctx, ptr(lb), V, n, C.byref(tok), ptr(p1), lp, C.byref(x), 0.0, 0.0, idp, len(ids)),
                         "dtk_op_sample_pen")
            model._check(model.lib.dtk_op_sample_ext(model._ctx, ptr(lb), V, n, C.byref(tok2), ptr(p2), lp2, C.byref(x)), "dtk_op_sample_ext")
            assert tok.value == tok2.value and p1.tobytes() == p2.tobytes() and bytes(lp) == bytes(lp2), (V, T, k, n)


# ------------------------------------------------------------------------------------------ one sequence, end to end
PP, FP = 0.6, 0.4


def _single(name):
    if name == "detikzify-tiny":
        from detikzify_amd.model import load
        model, proc = load(name, synthetic=1234)
        enc = proc(images=sketch_image(2, 96), return_tensors="pt")
        return model, enc.input_ids[0], enc.pixel_values, TINY.image_token_id
    model = _bigvocab()
    cfg = model.config
    ids = torch.tensor([cfg.image_token_id] * cfg.num_patches + [77, 30123, 9])
    return model, ids, torch.zeros(1, 3, cfg.vit_image, cfg.vit_image), cfg.image_token_id


@pytest.mark.parametrize("name", ["detikzify-tiny", "tiny-v2-40000"])
def test_generate_is_the_oracle_draw_over_the_device_logits(name):
    """24 tokens of generate(presence_penalty, frequency_penalty, temperature=1.2) == the same steps driven by hand, each of which is the
    oracle's draw over the row the device sampled from under the counts of the tokens generated so far (k_sample_fast on the toy
    vocabulary, the multi-block chain at 40 000); afterwards the device's table is the Counter of the 24 tokens"""
    model, ids, px, img = _single(name)
    T = int(ids.numel())
    out = model.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=24, eos_token_id=-1, bad_words_ids=[[img]], seed=31,
                         do_sample=True, temperature=1.2, top_k=0, presence_penalty=PP, frequency_penalty=FP)
    new = out[0, T:].tolist()
    assert len(new) == 24
    plain = model.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=24, eos_token_id=-1, bad_words_ids=[[img]], seed=31,
                           do_sample=True, temperature=1.2, top_k=0)[0, T:].tolist()
    assert model.token_counts().sum() == 0                    # the plain call reset the values: an empty table
    model.set_sampling(do_sample=True, temperature=1.2, seed=31, bad_ids=[img])
    model.set_penalties(PP, FP, T)
    model.prefill(ids, px)
    assert model.token_counts().sum() == 0                    # penalty_start = the prompt length: nothing counted yet
    made = []
    for n in range(24):
        row = model.get_logits()
        model.decode_launch()
        if n == 5:            # refused while a step is unread (DTK_ERR_STATE), and nothing changes
            assert model.lib.dtk_set_penalties(model._ctx, 1.0, 1.0, 0) == -3
        tok = model.decode_wait()
        want, _, _ = penalty_oracle.draw(row, made, PP, FP, 1.2, 0, 1.0, 31, n, bad=[img])
        assert tok == want == new[n], (name, n, tok, want, new[n])
        made.append(tok)
    counts = model.token_counts()
    ref = torch.zeros_like(counts)
    for t, c in Counter(made).items():
        ref[t] = c
    assert torch.equal(counts, ref)
    print(f"{name}: 24 tokens exact; {24 - len(set(made))} repeats; {sum(a != b for a, b in zip(new, plain))} of 24 differ from the run without penalties")
    assert new != plain
    # the values change on a live sequence: the table is rebuilt from its ids under the new start (here: the whole text)
    model.set_penalties(PP, FP, 0)
    full = Counter(ids.tolist() + made)
    c0 = model.token_counts()
    assert int(c0.sum()) == T + 24 and all(int(c0[t]) == c for t, c in full.items())
    del model
    gc.collect()


def test_greedy_leaves_its_loop():
    """the toy model's plain greedy run repeats a token within 24 steps; under the penalties every token is the oracle's arg-max of z'
    over the device's row, and the run is another one"""
    model, ids, px, img = _single("detikzify-tiny")
    T = int(ids.numel())
    kw = dict(input_ids=ids[None], pixel_values=px, max_new_tokens=24, eos_token_id=-1, bad_words_ids=[[img]], do_sample=False)
    plain = model.generate(**kw)[0, T:].tolist()
    assert len(set(plain)) < 24, plain
    pen = model.generate(presence_penalty=1.0, frequency_penalty=0.5, **kw)[0, T:].tolist()
    model.set_sampling(do_sample=False, bad_ids=[img])
    model.set_penalties(1.0, 0.5, T)
    model.prefill(ids, px)
    made = []
    for n in range(24):
        row = model.get_logits()
        model.decode_launch()
        tok = model.decode_wait()
        want = penalty_oracle.greedy(row, made, 1.0, 0.5, bad=[img])
        assert tok == want == pen[n], (n, tok, want, pen[n])
        made.append(tok)
    assert pen != plain
    print(f"greedy: plain run has {24 - len(set(plain))} repeats, penalised {24 - len(set(pen))}")
    del model
    gc.collect()


# ------------------------------------------------------------------------------------------ batched steps
TRIPLES = [(0.6, 0.4, None), (0.0, 0.0, None), (-0.5, -0.25, None), (1.5, 0.0, 0)]     # slot s: (presence, frequency, start; None: the prompt length)
STEPS = 12


def _prompts(proc, n):
    enc = proc(images=sketch_image(5, 96), return_tensors="pt")
    base, px = enc.input_ids[0], enc.pixel_values
    return [torch.cat([base, torch.tensor([20 + 3 * s, 41 + s][: 1 + s % 2], dtype=torch.int64)]) for s in range(n)], px


def _start(prompts, s):
    return int(prompts[s].numel()) if TRIPLES[s][2] is None else TRIPLES[s][2]


def _drive(model, prompts, px, slots, check):
    """STEPS batched steps of `slots` driven from the host; check: every token against the oracle's draw over the slot's own logits"""
    for s in slots:
        pp, fp, _ = TRIPLES[s]
        model.set_sampling(slot=s, do_sample=True, temperature=1.2, seed=900 + s, bad_ids=[TINY.image_token_id])
        if pp or fp:
            model.set_penalties(pp, fp, _start(prompts, s), slot=s)
        model.prefill(prompts[s], px, slot=s)
    toks = {s: [] for s in slots}
    for n in range(STEPS):
        rows = {s: model.get_logits_slot(s) for s in slots} if check else {}
        model.decode_batch_launch(slots)
        t = model.decode_batch_wait()
        for s in slots:
            if check:
                counted = prompts[s].tolist()[_start(prompts, s):] + toks[s]
                want, _, _ = penalty_oracle.draw(rows[s], counted, TRIPLES[s][0], TRIPLES[s][1], 1.2, 0, 1.0, 900 + s, n, bad=[TINY.image_token_id])
                assert t[s] == want, (s, n, t[s], want)
            toks[s].append(int(t[s]))
    if check:
        for s in slots:
            counted = Counter(prompts[s].tolist()[_start(prompts, s):] + toks[s]) if (TRIPLES[s][0] or TRIPLES[s][1]) else Counter()
            c = model.token_counts(slot=s)
            assert int(c.sum()) == sum(counted.values()) and all(int(c[t]) == k for t, k in counted.items()), s
    return toks


@pytest.fixture(scope="module", params=[5, 17], ids=["mv-4", "mfma-16"])
def batched(request):
    """detikzify-tiny with 5 slots (slots 0..3 decode with the multi-vector kernels) and with 17 (one MFMA column tile)"""
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny", synthetic=1234, batch_slots=request.param)
    assert model.max_decode_slots() == (4 if request.param == 5 else 16)
    prompts, px = _prompts(proc, 4)
    hand = _drive(model, prompts, px, [0, 1, 2, 3], check=True)       # (before anything switches the log-probabilities on)
    yield model, prompts, px, hand
    del model
    gc.collect()


def test_slots_with_their_own_values_are_exact_and_as_alone(batched):
    model, prompts, px, hand = batched
    for s in range(4):
        assert _drive(model, prompts, px, [s], check=False)[s] == hand[s], s
    # the values matter: slot 1 (0 / 0) is the plain sampler's sequence, and some other slot's is not what it would be without its values
    plain = {}
    for s in range(4):
        model.set_sampling(slot=s, do_sample=True, temperature=1.2, seed=900 + s, bad_ids=[TINY.image_token_id])
        model.prefill(prompts[s], px, slot=s)
    for n in range(STEPS):
        model.decode_batch_launch([0, 1, 2, 3])
        t = model.decode_batch_wait()
        for s in range(4):
            plain.setdefault(s, []).append(int(t[s]))
    assert plain[1] == hand[1]
    assert any(plain[s] != hand[s] for s in (0, 2, 3))


@pytest.mark.parametrize("engine", ["native", "python"])
def test_engines_carry_the_values_with_the_joins(batched, engine):
    """four sequences with their own values through either engine (one of them with return_logprobs): the tokens of the same slots driven
    by hand, which the fixture checked against the oracle; a later join without values inherits nothing"""
    from detikzify_amd.infer.batching import BatchEngine
    from detikzify_amd.infer.engine import NativeBatchEngine
    model, prompts, px, hand = batched
    model.enable_logprobs()
    eng = (NativeBatchEngine if engine == "native" else BatchEngine)(model, max_batch=4, share_prefix=False, resume_in_place=False)
    got, errs = {}, []
    common = dict(pixel_values=px, max_new_tokens=STEPS, eos_token_id=-1, bad_words_ids=[[TINY.image_token_id]], do_sample=True,
                  temperature=1.2, top_k=0)

    def run(s):
        try:
            pp, fp, st = TRIPLES[s]
            got[s] = model.generate(input_ids=prompts[s][None], seed=900 + s, presence_penalty=pp, frequency_penalty=fp, penalty_start=st,
                                    return_logprobs=(s == 0), **common)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    try:
        ths = [threading.Thread(target=run, args=(s,)) for s in range(4)]
        [t.start() for t in ths]
        [t.join(timeout=120) for t in ths]
        assert not any(t.is_alive() for t in ths) and not errs, errs[:1]
        again = model.generate(input_ids=prompts[0][None], seed=900, **common)
        again_pen = model.generate(input_ids=prompts[0][None], seed=900, presence_penalty=TRIPLES[0][0], frequency_penalty=TRIPLES[0][1], **common)
    finally:
        eng.close()
    T = [p.numel() for p in prompts]
    for s in range(4):
        seq = got[s].sequences if s == 0 else got[s]
        assert seq[0, T[s]:].tolist() == hand[s], (engine, s)
    out = got[0]
    assert out.sample_logprobs.shape == (1, STEPS) and bool(torch.isfinite(out.sample_logprobs).all()) and bool((out.sample_logprobs <= 0).all())
    assert again_pen[0, T[0]:].tolist() == hand[0]
    plain0 = again[0, T[0]:].tolist()
    model.set_sampling(slot=0, do_sample=True, temperature=1.2, seed=900, bad_ids=[TINY.image_token_id])
    model.prefill(prompts[0], px, slot=0)
    ref = []
    for n in range(STEPS):
        model.decode_batch_launch([0])
        ref.append(int(model.decode_batch_wait()[0]))
    assert plain0 == ref and plain0 != hand[0]


# ------------------------------------------------------------------------------------------ the chain, batched
def test_two_slots_of_the_chain_with_their_own_values():
    """the 40 000-token toy with slots: the multi-block chain under PN with a slot offset on pen / pen_cnt / pen_tok (sample_bind_slot) and
    k_count_token behind it for several slots.  6 steps of two slots under different values, every token the oracle's over the slot's own
    row, the tables read back; slot 1 counts from position 0 (the image placeholder, banned, counted num_patches times) with negative
    values"""
    model = _bigvocab(slots=3)
    cfg = model.config
    img = cfg.image_token_id
    px = torch.zeros(1, 3, cfg.vit_image, cfg.vit_image)
    prompts = [torch.tensor([img] * cfg.num_patches + [77, 30123, 9]), torch.tensor([img] * cfg.num_patches + [77, 8192, 39999, 8192])]
    vals = [(0.6, 0.4, int(prompts[0].numel())), (-0.5, -0.25, 0)]
    for s in (0, 1):
        model.set_sampling(slot=s, do_sample=True, temperature=1.2, top_p=0.95, seed=500 + s, bad_ids=[img])
        model.set_penalties(*vals[s], slot=s)
        model.prefill(prompts[s], px, slot=s)
    toks = {0: [], 1: []}
    for n in range(6):
        rows = {s: model.get_logits_slot(s) for s in (0, 1)}
        model.decode_batch_launch([0, 1])
        t = model.decode_batch_wait()
        for s in (0, 1):
            counted = prompts[s].tolist()[vals[s][2]:] + toks[s]
            want, _, _ = penalty_oracle.draw(rows[s], counted, vals[s][0], vals[s][1], 1.2, 0, 0.95, 500 + s, n, bad=[img])
            assert int(t[s]) == want, (s, n, int(t[s]), want)
            toks[s].append(int(t[s]))
    for s in (0, 1):
        counted = Counter(prompts[s].tolist()[vals[s][2]:] + toks[s])
        c = model.token_counts(slot=s)
        assert int(c.sum()) == sum(counted.values()) and all(int(c[k]) == v for k, v in counted.items()), s
    print(f"chain, 2 slots: 6 steps exact; slot 1 repeats {6 - len(set(toks[1]))} of its tokens")
    del model
    gc.collect()


# ------------------------------------------------------------------------------------------ the table follows the sequence
def test_the_table_follows_fork_resume_and_prefix_reuse():
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny", synthetic=1234, batch_slots=5)
    prompts, px = _prompts(proc, 1)
    prompt, img = prompts[0], TINY.image_token_id
    T = int(prompt.numel())
    key = model.image_key(px)

    def setup(s, seed):
        model.set_sampling(slot=s, do_sample=True, temperature=1.2, seed=seed, bad_ids=[img])
        model.set_penalties(PP, FP, T, slot=s)

    def table(counted):
        ref = torch.zeros(model.config.vocab, dtype=torch.int32)
        for t, c in Counter(counted).items():
            ref[t] = c
        return ref

    setup(0, 77)
    model.prefill(prompt, px, slot=0)
    made = []
    for n in range(8):
        model.decode_batch_launch([0])
        made.append(int(model.decode_batch_wait()[0]))
    ids = torch.cat([prompt, torch.tensor(made, dtype=torch.int64)])
    assert torch.equal(model.token_counts(slot=0), table(made))
    # fork: slot 1 takes the 8 generated tokens' counts with the KV; the prefill of the last token on top rebuilds the same table
    setup(1, 78)
    model.kv_fork(0, 1, int(ids.numel()))
    assert torch.equal(model.token_counts(slot=1), table(made))
    model.prefill(ids, px, slot=1, reuse=True)
    assert torch.equal(model.token_counts(slot=1), table(made))
    # resume: slot 2 holds the sequence from an earlier (plain) prefill; the forced last token is counted once, by the rebuild
    model.set_sampling(slot=2, do_sample=False)
    model.prefill(ids, px, slot=2)
    setup(2, 79)
    model.resume_slot(2, ids, key)
    assert torch.equal(model.token_counts(slot=2), table(made))
    model.set_penalties(PP, FP, T, slot=2)                        # values set again before the forced step: the forced id is still counted
    assert torch.equal(model.token_counts(slot=2), table(made))
    model.decode_batch_launch([1, 2])
    t = model.decode_batch_wait()
    assert int(t[2]) == made[-1]                                  # the forced token
    assert torch.equal(model.token_counts(slot=2), table(made))   # ... is not counted a second time
    rows = {2: model.get_logits_slot(2)}
    model.decode_batch_launch([2])
    t2 = model.decode_batch_wait()
    want2, _, _ = penalty_oracle.draw(rows[2], made, PP, FP, 1.2, 0, 1.0, 79, 0, bad=[img])
    assert int(t2[2]) == want2
    assert torch.equal(model.token_counts(slot=2), table(made + [want2]))
    # slot 1's first token after the fork: the oracle's over the row its prefill left (checked one step late: the row is gone after the step)
    setup(3, 78)
    model.kv_fork(0, 3, int(ids.numel()))
    model.prefill(ids, px, slot=3, reuse=True)
    row3 = model.get_logits_slot(3)
    model.decode_batch_launch([3])
    t3 = model.decode_batch_wait()
    want3, _, _ = penalty_oracle.draw(row3, made, PP, FP, 1.2, 0, 1.0, 78, 0, bad=[img])
    assert int(t3[3]) == want3 == int(t[1])                       # the same sequence, seed and counts as slot 1's step above
    # a DTK_PREFILL_REUSE_PREFIX prefill of a shorter prompt drops the counts of the cut tokens
    model.prefill(ids[:T + 3], px, slot=0, reuse=True)
    assert torch.equal(model.token_counts(slot=0), table(made[:3]))
    del model
    gc.collect()
