"""Top-k alternatives on the MI355X: dtk_op_score_top against the GEMM kernel's own logits (exact), model.score / score_candidates
with top_logprobs, the decode step's k_top_logits (single sequence and both batched families), generate and the pipeline.
Every expected value is tests/test_topk_host.ordered_topk of logits the device itself wrote."""
from __future__ import annotations

import ctypes as C
import gc
import math

import numpy as np
import pytest
import torch

from oracle.ops import bits_to_f32, f32_to_bits, rb
from tests.helpers import TINY, sketch_image
from tests.test_topk_host import ordered_topk

pytestmark = pytest.mark.gpu
SAMPLED = dict(do_sample=True, temperature=0.8, top_p=0.95)


@pytest.fixture(scope="module")
def tiny():
    from detikzify_amd.model import load
    return load("detikzify-tiny", synthetic=1234)


def _topk_rows(rows, k):
    ids, vals = zip(*(ordered_topk(r, k) for r in np.asarray(rows)))
    return np.stack(ids), np.stack(vals)


# ------------------------------------------------------------------------------------------ the kernel pair alone
_OP_REF = {}


def _op_case(model, M, N, K, wt):
    """operands with both planted ties + dtk_op_gemm's own z, computed once per shape"""
    key = (M, N, K, wt)
    if key not in _OP_REF:
        g = torch.Generator().manual_seed(M + N + K)
        A = rb(torch.randn(M, K, generator=g)); W = rb(torch.randn(N, K, generator=g) * 0.3)
        W[N // 3] = W[N // 3 + 5]
        W[122:133] = W[122].clone()                    # eleven identical rows that straddle the boundary of tiles 0 and 1
        for r, f in ((1, 2.0), (M // 2, 4.0), (M - 1, 8.0)):
            A[r] = rb(W[122] * f)                      # a positive multiple: these rows' maxima are the eleven equal logits
        tg = torch.randint(0, N, (M,), generator=g, dtype=torch.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        Ab, Wb, Tb = f32_to_bits(A), f32_to_bits(W), tg.numpy()
        z = np.empty((M, N), dtype=np.uint16)
        model._check(model.lib.dtk_op_gemm(model._ctx, p(Ab), p(Wb), None, None, M, N, K, 0, p(z)), "dtk_op_gemm")
        zf = bits_to_f32(z).numpy()
        _OP_REF[key] = (Ab, Wb, Tb, zf, torch.logsumexp(torch.from_numpy(zf).double(), dim=-1).numpy())
    return _OP_REF[key]


@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("M,N,K,wt", [(37, 1000, 64, 0), (130, 515, 304, 0), (300, 16424, 128, 0), (70, 16424, 192, 1), (70, 16424, 200, 1)])
def test_op_score_top_against_the_gemm_kernels_own_logits(tiny, M, N, K, wt, k):
    from detikzify_amd import _lib
    model, _ = tiny
    Ab, Wb, Tb, zf, lse64 = _op_case(model, M, N, K, wt)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    flags = _lib.DTK_GEMM_WT if wt else 0
    lp, lse, am, zm = np.empty(M, np.float32), np.empty(M, np.float32), np.empty(M, np.int32), np.empty(M, np.float32)
    ti, tl, tz = np.empty((M, k), np.int32), np.empty((M, k), np.float32), np.empty((M, k), np.float32)
    model._check(model.lib.dtk_op_score_top(model._ctx, p(Ab), p(Wb), p(Tb), M, N, K, flags, p(lp), p(lse), p(am), p(zm), k, p(ti), p(tl), p(tz)),
                 "dtk_op_score_top")
    want_ids, want_z = _topk_rows(zf, k)
    tied = [r for r in (1, M // 2, M - 1) if (zf[r, 122:133] == zf[r].max()).all()]
    assert tied, "the planted rows were to have eleven equal maxima"
    assert np.array_equal(ti, want_ids), np.argwhere(ti != want_ids)[:4]
    assert np.array_equal(tz, want_z)
    assert np.array_equal(ti[:, 0], am) and np.array_equal(tz[:, 0], zm)
    d = float(np.abs(tl.astype(np.float64) - (want_z.astype(np.float64) - lse64[:, None])).max())
    print(f"op_score_top {M}x{N}x{K} wt={wt} k={k}: max |d top_logprob| {d:.2e}; rows with eleven equal maxima: {tied}")
    assert d <= 2e-5
    assert np.array_equal(tl, tz - lse[:, None])                  # the entry's logprob is z - the call's own lse, as logprob is
    hit = ti == Tb[:, None]
    assert np.array_equal(tl[hit], np.broadcast_to(lp[:, None], tl.shape)[hit])
    # no dependence on M
    M2 = max(1, M // 3)
    ti2, tl2, tz2, lp2 = np.empty((M2, k), np.int32), np.empty((M2, k), np.float32), np.empty((M2, k), np.float32), np.empty(M2, np.float32)
    model._check(model.lib.dtk_op_score_top(model._ctx, p(Ab), p(Wb), p(Tb), M2, N, K, flags, p(lp2), None, None, None, k, p(ti2), p(tl2), p(tz2)),
                 "dtk_op_score_top")
    assert np.array_equal(ti2, ti[:M2]) and np.array_equal(tl2, tl[:M2]) and np.array_equal(tz2, tz[:M2])
    # k = 0 with NULL outputs is dtk_op_score
    a0, b0 = [np.empty(M, np.float32), np.empty(M, np.float32), np.empty(M, np.int32)], [np.empty(M, np.float32), np.empty(M, np.float32), np.empty(M, np.int32)]
    model._check(model.lib.dtk_op_score_top(model._ctx, p(Ab), p(Wb), p(Tb), M, N, K, flags, p(a0[0]), p(a0[1]), p(a0[2]), None, 0, None, None, None), "dtk_op_score_top")
    model._check(model.lib.dtk_op_score(model._ctx, p(Ab), p(Wb), p(Tb), M, N, K, flags, p(b0[0]), p(b0[1]), p(b0[2]), None), "dtk_op_score")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a0, b0)) and a0[0].tobytes() == lp.tobytes() and a0[1].tobytes() == lse.tobytes()


def test_op_score_top_refuses_bad_k(tiny):
    model, _ = tiny
    z = np.zeros(64, np.uint16); t = np.zeros(1, np.int32); o = np.zeros(16, np.float32); oi = np.zeros(16, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for k, a, b in ((9, p(oi), p(o)), (3, None, p(o)), (0, p(oi), p(o)), (5, p(oi), p(o))):      # (5 > N = 4)
        assert model.lib.dtk_op_score_top(model._ctx, p(z), p(z), p(t), 1, 4, 8, 0, p(o), None, None, None, k, a, b, None) == -1


# ------------------------------------------------------------------------------------------ model.score
def _program(model, proc, n, seed):
    enc = proc(images=sketch_image(3, 96), return_tensors="pt")
    prog = torch.randint(3, model.config.vocab - 1, (n,), generator=torch.Generator().manual_seed(seed))
    prog = prog[prog != model.config.image_token_id]
    return enc.input_ids[0], prog, enc.pixel_values


@pytest.mark.parametrize("name", ["detikzify-tiny", "detikzify-tiny-tl"])
def test_model_score_top(name, tiny):
    """score(top_logprobs=5): the old fields keep their bits; at four positions the ids are the ordered top-5 of the logits one prefill
    per position gives, exactly: test_score_agrees_with_one_prefill_per_position needs no near-tie rule, so none is applied here
    (measured on an MI355X: 0 of 20 entries differ, for both presets)."""
    from detikzify_amd.model import load
    model, proc = tiny if name == "detikzify-tiny" else load(name, synthetic=1234)
    prompt, prog, px = _program(model, proc, 24, 11)
    ids = torch.cat([prompt, prog])
    first = prompt.numel()
    ids[-1] = model.score(ids, px, first=first).argmax[-1]      # the last target is its position's arg-max: at least one target is among the ids
    plain = model.score(ids, px, first=first)
    assert plain.top_ids is None and plain.top_logprobs is None
    out = model.score(ids, px, first=first, top_logprobs=5)
    n = ids.numel() - first
    assert out.top_ids.shape == out.top_logprobs.shape == (n, 5) and out.top_ids.dtype == torch.int64 and out.top_logprobs.dtype == torch.float32
    for f in ("logprobs", "argmax", "lse"):
        assert torch.equal(getattr(out, f), getattr(plain, f)), f
    assert torch.equal(out.top_ids[:, 0], out.argmax)
    assert bool((out.top_logprobs[:, :-1] >= out.top_logprobs[:, 1:]).all())
    hit = out.top_ids == ids[first:, None]
    assert bool(hit[-1, 0])
    assert torch.equal(out.top_logprobs[hit], out.logprobs[:, None].expand(-1, 5)[hit])
    for t in (first, first + n // 3, first + (2 * n) // 3, ids.numel() - 1):
        row = model.prefill(ids[:t], px, return_logits=True).numpy()
        assert out.top_ids[t - first].tolist() == ordered_topk(row, 5)[0].tolist(), t


def test_score_candidates_top(tiny):
    model, proc = tiny
    prompt, prog, px = _program(model, proc, 30, 12)
    cands = [prog[:9], prog[9:14], prog[14:]]
    outs = model.score_candidates(prompt, cands, px, top_logprobs=3)
    P = prompt.numel()
    for c, o in zip(cands, outs):
        one = model.score(torch.cat([prompt, c]), px, first=P, top_logprobs=3)
        assert o.top_ids.shape == (c.numel(), 3)
        assert torch.equal(o.logprobs, one.logprobs) and torch.equal(o.argmax, one.argmax)
        assert torch.equal(o.top_ids, one.top_ids) and torch.equal(o.top_logprobs, one.top_logprobs)
    plain = model.score_candidates(prompt, cands, px)
    assert all(o.top_ids is None for o in plain) and all(torch.equal(a.logprobs, b.logprobs) for a, b in zip(plain, outs))


# ------------------------------------------------------------------------------------------ decode, one sequence
def _run_single(model, ids, px, steps, k, sampling):
    """tokens, lp pairs and — k > 0 — the top-k of every step next to the logits row the step sampled from"""
    model.set_sampling(**sampling)
    model.enable_logprobs()
    model.enable_top_logprobs(k)
    model.prefill(ids, px)
    out = []
    for _ in range(steps):
        row = model.get_logits().numpy().copy()
        model.decode_launch()
        if k:
            tok, lp, slp, ti, tl = model.decode_wait(top=True)
        else:
            (tok, lp, slp), ti, tl = model.decode_wait_lp(), None, None
        out.append((tok, lp, slp, ti, tl, row))
    return out


@pytest.mark.parametrize("mode", ["sampled", "greedy"])
def test_decode_single_sequence(mode):
    """the toy vocabulary runs k_sample_fast in a step; k_sample and the multi-block chain: test_decode_big_vocabulary_families"""
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny", synthetic=1234)
    enc = proc(images=sketch_image(4, 96), return_tensors="pt")
    ids, px = enc.input_ids[0], enc.pixel_values
    base = dict(seed=55, bad_ids=[TINY.image_token_id], **(SAMPLED if mode == "sampled" else dict(do_sample=False)))
    first_row = model.prefill(ids, px, return_logits=True).numpy()
    top = int(np.argsort(-first_row.astype(np.float64), kind="stable")[0])
    for tag, samp in (("plain", base), ("argmax suppressed", dict(base, bad_ids=[TINY.image_token_id, top]))):
        k = 5
        on = _run_single(model, ids, px, 12, k, samp)
        off = _run_single(model, ids, px, 12, 0, samp)
        assert [(a[0], a[1], a[2]) for a in on] == [(a[0], a[1], a[2]) for a in off], tag
        for step, (tok, lp, slp, ti, tl, row) in enumerate(on):
            want, wz = ordered_topk(row, k)
            assert ti == want.tolist(), (tag, step)
            lse = float(torch.logsumexp(torch.from_numpy(row).double(), 0))
            assert max(abs(a - (float(z) - lse)) for a, z in zip(tl, wz)) <= 2e-5
            if tok in ti:
                assert tl[ti.index(tok)] == lp
            if mode == "greedy" and tag == "plain" and TINY.image_token_id != ti[0]:
                assert tok == ti[0]
        if tag != "plain":
            assert on[0][3][0] == top and on[0][0] != top      # the suppressed arg-max still leads the top-k; it was not chosen
    model.enable_top_logprobs(0)
    model.decode_launch()
    tok, lp = C.c_int64(), (C.c_float * 2)()
    ti, tl = (C.c_int32 * 8)(), (C.c_float * 8)()
    assert model.lib.dtk_decode_wait_top(model._ctx, C.byref(tok), lp, ti, tl) == -1 and b"top_logprobs" in model.lib.dtk_last_error(model._ctx)
    assert model.decode_wait() >= 0
    model.enable_top_logprobs(2)
    from detikzify_amd import _lib
    with pytest.raises(_lib.DtkError):
        model.set_option("logprobs", 0)
    with pytest.raises(_lib.DtkError):
        model.set_option("top_logprobs", 9)


# ------------------------------------------------------------------------------------------ decode, batched steps
@pytest.mark.parametrize("n,slots", [(16, [0, 5, 11]), (4, [1, 3])], ids=["mfma-16", "mv-4"])
def test_decode_batched_step(n, slots):
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny", synthetic=1234, batch_slots=n + 1)
    assert model.max_decode_slots() == n
    enc = proc(images=sketch_image(7, 96), return_tensors="pt")
    base, px = enc.input_ids[0], enc.pixel_values
    k = 4
    runs = {}
    for kk in (k, 0):
        model.enable_logprobs()
        model.enable_top_logprobs(kk)
        for s in slots:
            model.set_sampling(slot=s, seed=900 + s, bad_ids=[TINY.image_token_id], **(SAMPLED if s != slots[0] else dict(do_sample=False)))
            model.prefill(torch.cat([base, torch.tensor([20 + s])]), px, slot=s)
        steps = []
        for _ in range(6):
            rows = {s: model.get_logits_slot(s).numpy().copy() for s in slots}
            model.decode_batch_launch(slots)
            if kk:
                t, lp, slp, ti, tl = model.decode_batch_wait(top=True)
                for s in range(64):
                    if s not in slots:
                        assert t[s] == -1 and ti[s] == [-1] * k and all(math.isnan(v) for v in tl[s])
                for s in slots:
                    want, wz = ordered_topk(rows[s], k)
                    assert ti[s] == want.tolist(), s
                    lse = float(torch.logsumexp(torch.from_numpy(rows[s]).double(), 0))
                    assert max(abs(a - (float(z) - lse)) for a, z in zip(tl[s], wz)) <= 2e-5
                    if t[s] in ti[s]:
                        assert tl[s][ti[s].index(t[s])] == lp[s]
                g = slots[0]                                 # the greedy slot
                if ti[g][0] != TINY.image_token_id:
                    assert t[g] == ti[g][0]
            else:
                t, lp, slp = model.decode_batch_wait_lp()
            steps.append([(t[s], lp[s], slp[s]) for s in slots])
        runs[kk] = steps
    assert runs[k] == runs[0]
    del model
    gc.collect()


# ------------------------------------------------------------------------------------------ the other sampler families in a step
@pytest.fixture(scope="module", params=[5, 17], ids=["mv-4", "mfma-16"])
def bigvocab(request):
    """tiny-v2 with a 40 000-token vocabulary, as tests/test_gpu_parity.py builds it: top_k = 0 takes the multi-block chain (k_smb_*),
    top_k = 50 takes k_sample, in the single-sequence step and in the batched step of either family"""
    from detikzify_amd.model.config import preset
    from detikzify_amd.model.modeling import DetikzifyForCausalLM
    cfg = preset("detikzify-tiny-v2")
    cfg.vocab, cfg.name_or_path, cfg.batch_slots = 40000, "detikzify-tiny-v2-bigvocab", request.param
    m = DetikzifyForCausalLM(cfg, 0)
    m.fill_synthetic(99)
    yield m
    del m
    gc.collect()


def _check_step(tag, row, tok, lp, ti, tl, k):
    want, wz = ordered_topk(row, k)
    assert ti == want.tolist(), tag
    lse = float(torch.logsumexp(torch.from_numpy(row).double(), 0))
    assert max(abs(a - (float(z) - lse)) for a, z in zip(tl, wz)) <= 2e-5, tag
    if tok in ti:
        assert tl[ti.index(tok)] == lp, tag        # the stored logsumexp is the one the token's logprob was taken against
    return tok in ti


@pytest.mark.parametrize("family,top_k", [("multi-block", 0), ("k_sample", 50)])
def test_decode_big_vocabulary_families(bigvocab, family, top_k):
    model = bigvocab
    cfg = model.config
    ids = torch.tensor([cfg.image_token_id] * cfg.num_patches + [77, 30123, 9])
    px = torch.zeros(1, 3, cfg.vit_image, cfg.vit_image)
    k = 5
    first_row = model.prefill(ids, px, return_logits=True).numpy()
    top = int(ordered_topk(first_row, 1)[0][0])
    hits = 0
    for mode in ("sampled", "greedy"):
        base = dict(do_sample=True, temperature=0.8, top_p=0.95, top_k=top_k, seed=4) if mode == "sampled" else dict(do_sample=False)
        for tag, bad in (("plain", [cfg.image_token_id]), ("argmax suppressed", [cfg.image_token_id, top])):
            samp = dict(base, bad_ids=bad, begin_suppress_ids=[2])
            on = _run_single(model, ids, px, 12, k, samp)
            off = _run_single(model, ids, px, 12, 0, samp)
            assert [a[:3] for a in on] == [a[:3] for a in off], (family, mode, tag)
            for step, (tok, lp, slp, ti, tl, row) in enumerate(on):
                hits += _check_step((family, mode, tag, step), row, tok, lp, ti, tl, k)
                if mode == "greedy" and tag == "plain" and ti[0] not in (cfg.image_token_id, 2):
                    assert tok == ti[0]
            if tag != "plain":
                assert on[0][3][0] == top and on[0][0] != top
    assert hits > 0, "no sampled token was among its position's top-k: the bit-equality was never checked"
    # the batched step of this context's family: slot 0 greedy, the others sampled
    slots = [0, 2, 3]
    runs = {}
    for kk in (k, 0):
        model.enable_top_logprobs(kk)
        for s in slots:
            model.set_sampling(slot=s, seed=900 + s, bad_ids=[cfg.image_token_id], begin_suppress_ids=[2],
                               **(dict(do_sample=True, temperature=0.8, top_p=0.95, top_k=top_k) if s else dict(do_sample=False)))
            model.prefill(torch.cat([ids, torch.tensor([20 + s])]), px, slot=s)
        steps = []
        for i in range(6):
            rows = {s: model.get_logits_slot(s).numpy().copy() for s in slots}
            model.decode_batch_launch(slots)
            if kk:
                t, lp, slp, ti, tl = model.decode_batch_wait(top=True)
                for s in range(64):
                    if s not in slots:
                        assert t[s] == -1 and ti[s] == [-1] * k and all(math.isnan(v) for v in tl[s])
                for s in slots:
                    hits += _check_step((family, "batched", s, i), rows[s], t[s], lp[s], ti[s], tl[s], k)
                if ti[0][0] not in (cfg.image_token_id, 2):
                    assert t[0] == ti[0][0]
            else:
                t, lp, slp = model.decode_batch_wait_lp()
            steps.append([(t[s], lp[s], slp[s]) for s in slots])
        runs[kk] = steps
    assert runs[k] == runs[0]
    model.enable_top_logprobs(0)


# ------------------------------------------------------------------------------------------ generate, pipeline
def test_generate_and_pipeline(tiny):
    from detikzify_amd.infer.pipeline import DetikzifyPipeline
    model, proc = tiny
    enc = proc(images=sketch_image(2, 96), return_tensors="pt")
    kw = dict(input_ids=enc.input_ids, pixel_values=enc.pixel_values, max_new_tokens=20, eos_token_id=-1,
              bad_words_ids=[[TINY.image_token_id]], seed=31, return_logprobs=True, **SAMPLED)
    plain = model.generate(**kw)
    out = model.generate(top_logprobs=4, **kw)
    assert plain.top_ids is None
    assert out.top_ids.shape == out.top_logprobs.shape == (1, 20, 4) and out.top_ids.dtype == torch.int64
    assert torch.equal(out.sequences, plain.sequences) and torch.equal(out.logprobs, plain.logprobs)
    assert torch.equal(out.sample_logprobs, plain.sample_logprobs)
    assert bool((out.top_logprobs[..., :-1] >= out.top_logprobs[..., 1:]).all())
    assert model.top_logprobs_enabled == 0              # the call that asked switched it off again
    again = model.generate(**kw)
    assert torch.equal(again.logprobs, plain.logprobs)
    pipe = DetikzifyPipeline(model, proc, metric="fast", max_length=enc.input_ids.shape[1] + 12)
    doc = pipe.sample(image=sketch_image(2, 96), return_logprobs=True, top_logprobs=4)
    n = len(doc.token_logprobs)
    assert n > 0 and len(doc.token_top_ids) == len(doc.token_top_logprobs) == n and all(len(r) == 4 for r in doc.token_top_ids)
