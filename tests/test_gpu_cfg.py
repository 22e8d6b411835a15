"""Classifier-free guidance on the device (dtk_set_guidance): the two mixing kernels op by op against float64 and
against the float32 replay of their own arithmetic, a guided pair of slots step by step against the sampling oracle over the mixed
row (multi-vector and MFMA families), placement and company, the refusals, and generate(guidance_scale=...) end to end."""
from __future__ import annotations

import ctypes as C
import gc

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from oracle import sampling
from tests import cfg_oracle, shape_oracle
from tests.helpers import TINY, sketch_image

pytestmark = pytest.mark.gpu

F32P = C.POINTER(C.c_float)
IMG = TINY.image_token_id
# 8: one ragged group of one slice; 512 / 1000: one slice; 1003: rows at stride V that are not 16-byte aligned, ragged tail; 1030: two
# slices; 32 024: the v1 vocabularies; 128 256: v2's (126 slices)
VS = [8, 512, 1000, 1003, 1030, 32024, 128256]
GS = [0.0, 0.5, 1.5, 3.0, 7.5]
LSE_TOL = 2e-5
WORST = {"lse": 0.0}


def _load(slots):
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny", synthetic=1234, batch_slots=slots)
    model.enable_logprobs()
    return model, proc


def op_mix(model, zc, zu, g):
    """dtk_op_cfg_mix: (out float32 [V], (Lc, Lu) float32)"""
    zc, zu = np.ascontiguousarray(zc, dtype=np.float32), np.ascontiguousarray(zu, dtype=np.float32)
    out, lse = np.empty_like(zc), np.zeros(2, dtype=np.float32)
    rc = model.lib.dtk_op_cfg_mix(model._ctx, zc.ctypes.data_as(C.c_void_p), zu.ctypes.data_as(C.c_void_p), zc.size, float(g),
                                  out.ctypes.data_as(C.c_void_p), lse.ctypes.data_as(F32P))
    model._check(rc, "dtk_op_cfg_mix")      # (a written guard byte behind out is DTK_ERR_STATE)
    return out, lse


@pytest.fixture(scope="module")
def mv():
    """detikzify-tiny with 5 slots: slots 0..3 decode with the multi-vector kernels"""
    model, proc = _load(5)
    assert model.max_decode_slots() == 4
    yield model, proc
    del model
    gc.collect()


@pytest.fixture(scope="module", params=[5, 16], ids=["mv-4", "mfma-16"])
def family(request, mv):
    if request.param == 5:
        yield mv
        return
    model, proc = _load(16)
    assert model.max_decode_slots() == 16
    yield model, proc
    del model
    gc.collect()


# ------------------------------------------------------------------------------------------ the two mixing kernels, op by op
@pytest.fixture(scope="module")
def rows():
    """seeded normal rows of scale 1 and of scale 8, and their float64 logsumexp, per V: computed once"""
    out = {}
    for V in VS:
        rng = np.random.default_rng(1000 + V)
        for scale in (1.0, 8.0):
            zc = (rng.standard_normal(V) * scale).astype(np.float32)
            zu = (rng.standard_normal(V) * scale).astype(np.float32)
            out[V, scale] = (zc, zu, cfg_oracle.lse64(zc), cfg_oracle.lse64(zu))
    return out


@pytest.mark.parametrize("V", VS)
def test_op_mix_against_float64_and_its_own_replay(mv, rows, V):
    model, _ = mv
    for scale in (1.0, 8.0):
        zc, zu, Lc64, Lu64 = rows[V, scale]
        for g in GS:
            out, lse = op_mix(model, zc, zu, g)                                        # (f): the guard bytes behind out are intact, or this raises
            ec, eu = abs(float(lse[0]) - Lc64), abs(float(lse[1]) - Lu64)
            WORST["lse"] = max(WORST["lse"], ec, eu)
            print(f"V={V} scale={scale} g={g}: |Lc - Lc64| = {ec:.3g}, |Lu - Lu64| = {eu:.3g}")
            assert ec <= LSE_TOL and eu <= LSE_TOL, (V, scale, g, ec, eu)                 # (a)
            assert out.tobytes() == cfg_oracle.out32(zc, zu, g, lse[0], lse[1]).tobytes(), (V, scale, g)      # (b)
            if g == GS[0]:
                assert out.tobytes() == (zu - lse[1]).tobytes()                           # (d) g = 0: zu - Lu
            if g in (GS[0], GS[-1]):
                again, lse2 = op_mix(model, zc, zu, g)
                assert again.tobytes() == out.tobytes() and lse2.tobytes() == lse.tobytes()      # (c)
            same, l2 = op_mix(model, zc, zc, g)                                           # (d) zu = zc: zc - Lc for every g
            assert l2[0].tobytes() == l2[1].tobytes() == lse[0].tobytes()                 # (the same row in either place: the same bits)
            assert same.tobytes() == (zc - l2[0]).tobytes(), (V, scale, g)
    print(f"worst |L - L64| so far: {WORST['lse']:.3g}")


@pytest.mark.parametrize("V", [8, 1003, 32024, 128256])
def test_op_mix_stays_finite_on_a_row_of_range_160(mv, V):
    model, _ = mv
    zc, zu = np.full(V, -80.0, dtype=np.float32), np.full(V, -80.0, dtype=np.float32)
    zc[V // 3], zu[V - 1] = 80.0, 80.0
    for g in (0.0, 1.5, 7.5, 100.0):
        out, lse = op_mix(model, zc, zu, g)
        assert np.isfinite(out).all() and np.isfinite(lse).all() and abs(float(lse[0]) - 80.0) <= LSE_TOL and abs(float(lse[1]) - 80.0) <= LSE_TOL
        assert out.tobytes() == cfg_oracle.out32(zc, zu, g, lse[0], lse[1]).tobytes()


def test_op_mix_refuses_bad_arguments(mv):
    model, _ = mv
    z = np.zeros(16, dtype=np.float32)
    for g in (-0.5, 100.5, float("nan"), float("inf")):
        with pytest.raises(Exception):
            op_mix(model, z, z, g)
    out, lse = op_mix(model, z, z, 2.0)
    assert abs(float(lse[0]) - np.log(16.0)) < 1e-6


# ------------------------------------------------------------------------------------------ a guided pair, step by step
STEPS = 12
G = 2.0
GREEDY = dict(do_sample=False)
SAMPLED = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=4711)


def _prompts(proc):
    a, b = proc(images=sketch_image(2, 96), return_tensors="pt"), proc(images=sketch_image(7, 96), return_tensors="pt")
    tail = torch.tensor([77, 30, 9], dtype=torch.int64)
    return torch.cat([a.input_ids[0], tail]), a.pixel_values, b.pixel_values


def _pick(row, cfg, n, cur, **shape):
    """the oracle's token over the (mixed) row: draw index n, sequence length cur"""
    row = torch.from_numpy(np.asarray(row, dtype=np.float32).copy())
    if shape:
        if cfg["do_sample"]:
            return shape_oracle.draw(row, cur, cfg["temperature"], cfg["top_k"], cfg["top_p"], cfg["seed"], n, bad=[IMG], **shape)[0]
        return shape_oracle.greedy(row, cur, bad=[IMG], **shape)
    if cfg["do_sample"]:
        return sampling.draw(row, cfg["temperature"], cfg["top_k"], cfg["top_p"], cfg["seed"], n, bad=[IMG])[0]
    return sampling.greedy(row, bad=[IMG])


def _pair_by_hand(model, c, u, ids, px, px2, cfg, g=G, steps=STEPS, topk=0, company=None, pp=0.0, pairs=None):
    """the pair (c, u) stepped by hand: before each launch both pending rows are read back and mixed by dtk_op_cfg_mix (the same
    kernels, hence the same bits as the step's); both slots' tokens must be the oracle's pick over that row, the log-probability the
    float64 log-softmax of that row at the token.  company: an unguided slot decoding beside the pair.  pp / pairs: a presence
    penalty and a logit bias on the conditional slot.  Returns (tokens, logprob bits, company's tokens)"""
    T = int(ids.numel())
    model.set_sampling(slot=c, bad_ids=[IMG], **cfg)
    if pp:
        model.set_penalties(pp, 0.0, T, slot=c)
    if pairs:
        model.set_logit_bias(pairs, slot=c)
    model.set_sampling(slot=u)
    active = [c, u]
    if company is not None:
        model.set_sampling(slot=company, bad_ids=[IMG], **{**cfg, "seed": 99} if cfg["do_sample"] else cfg)
        model.prefill(ids, px2, slot=company)
        active.append(company)
    model.prefill(ids, px, slot=c)
    model.prefill(ids, px2, slot=u)
    model.enable_top_logprobs(topk)
    model.set_guidance(g, c, u)
    toks, bits, beside = [], [], []
    shape = dict(pairs=pairs, pp=pp) if (pp or pairs) else {}
    try:
        for n in range(steps):
            zc, zu = model.get_logits_slot(c).numpy(), model.get_logits_slot(u).numpy()
            mixed, lse = op_mix(model, zc, zu, g)
            model.decode_batch_launch(sorted(active))
            if topk:
                t, lp, slp, ti, tl = model.decode_batch_wait(top=True)
            else:
                t, lp, slp = model.decode_batch_wait_lp()
            want = _pick(mixed, cfg, n, T + n, **({**shape, "counted": toks} if shape else {}))
            assert t[c] == want and t[u] == want, (n, t[c], t[u], want)
            ref = cfg_oracle.logprob64(mixed, want)
            assert abs(lp[c] - ref) <= LSE_TOL, (n, lp[c], ref)
            assert np.float32(lp[u]).tobytes() == np.float32(lp[c]).tobytes()          # the follower copied the ring entries
            got = model.guidance(c)["lse"]
            assert np.float32(got[0]).tobytes() == lse[0].tobytes() and np.float32(got[1]).tobytes() == lse[1].tobytes()
            if topk:
                order = np.argsort(-mixed.astype(np.float64), kind="stable")[:topk]
                assert list(ti[c]) == order.tolist() and list(ti[u]) == order.tolist(), n
                if want in ti[c]:       # the chosen token's entry is its logprob, bit for bit
                    assert np.float32(tl[c][list(ti[c]).index(want)]).tobytes() == np.float32(lp[c]).tobytes(), n
            toks.append(int(want))
            bits.append(np.float32(lp[c]).tobytes())
            if company is not None:
                beside.append(int(t[company]))
    finally:
        model.set_guidance(None, c, None)
        model.enable_top_logprobs(0)
    return toks, bits, beside


@pytest.mark.parametrize("cfg", [GREEDY, SAMPLED], ids=["greedy", "sampled"])
def test_a_guided_pair_is_the_oracle_over_the_mixed_row(family, cfg):
    model, proc = family
    ids, px, px2 = _prompts(proc)
    toks, bits, _ = _pair_by_hand(model, 0, 1, ids, px, px2, cfg)
    # the guidance matters: the unguided slot's sequence is another one
    model.set_sampling(slot=0, bad_ids=[IMG], **cfg)
    model.prefill(ids, px, slot=0)
    alone = []
    for n in range(STEPS):
        model.decode_batch_launch([0])
        alone.append(model.decode_batch_wait()[0])
    assert alone != toks
    # with the alternatives on: the records are the mixed row's, the chosen token's entry equals .logprobs
    again, bits2, _ = _pair_by_hand(model, 0, 1, ids, px, px2, cfg, topk=4)
    assert again == toks and bits2 == bits
    assert model.guidance(0) is None and model.guidance(1) is None


def test_placement_and_company(family):
    model, proc = family
    ids, px, px2 = _prompts(proc)
    base, bits, _ = _pair_by_hand(model, 0, 1, ids, px, px2, SAMPLED)
    moved, mbits, _ = _pair_by_hand(model, 3, 2, ids, px, px2, SAMPLED)
    assert moved == base and mbits == bits
    # an unguided third sequence beside the pair draws what it draws alone, and the pair what it draws alone
    cfg3 = {**SAMPLED, "seed": 99}
    model.set_sampling(slot=2, bad_ids=[IMG], **cfg3)
    model.prefill(ids, px2, slot=2)
    alone = []
    for n in range(STEPS):
        model.decode_batch_launch([2])
        alone.append(model.decode_batch_wait()[2])
    paired, pbits, beside = _pair_by_hand(model, 0, 1, ids, px, px2, SAMPLED, company=2)
    assert beside == alone and paired == base and pbits == bits


def test_refusals(family):
    model, proc = family
    ids, px, px2 = _prompts(proc)
    lib, ctx = model.lib, model._ctx
    for s in (0, 1, 2, 3):
        model.set_sampling(slot=s)
        model.prefill(ids, px if s % 2 == 0 else px2, slot=s)
    assert lib.dtk_set_guidance(ctx, 0, 0, 2.0) == -1                                   # equal slots
    assert lib.dtk_set_guidance(ctx, 0, 99, 2.0) == -1 and lib.dtk_set_guidance(ctx, 99, 0, 2.0) == -1
    for g in (-0.1, 100.5, float("nan"), float("inf")):
        assert lib.dtk_set_guidance(ctx, 0, 1, g) == -1
    assert model.guidance(0) is None
    model.set_guidance(2.0, 0, 1)
    assert model.guidance(0) == dict(partner=1, is_cond=True, scale=2.0, lse=model.guidance(0)["lse"])
    assert model.guidance(1)["partner"] == 0 and not model.guidance(1)["is_cond"]
    assert lib.dtk_set_guidance(ctx, 2, 1, 2.0) == -1 and lib.dtk_set_guidance(ctx, 1, 3, 2.0) == -1      # a slot already in another pair
    assert lib.dtk_set_guidance(ctx, 2, 0, 2.0) == -1
    assert b"already in the pair (0, 1)" in lib.dtk_last_error(ctx)
    model.set_guidance(3.0, 0, 1)                                                        # the pair again: a new scale
    assert model.guidance(0)["scale"] == 3.0
    model.set_guidance(1.5, 3, 2)                                                        # a second, disjoint pair
    # a launch with one slot of a pair active: refused, the pair named, nothing launched; the next full launch works
    arr = (C.c_int32 * _lib.DTK_MAX_BATCH)()
    arr[0] = 1
    assert lib.dtk_decode_batch_launch(ctx, arr) == -1
    assert b"guided pair (0, 1)" in lib.dtk_last_error(ctx)
    arr[0], arr[2] = 0, 1
    assert lib.dtk_decode_batch_launch(ctx, arr) == -1 and b"guided pair (3, 2)" in lib.dtk_last_error(ctx)
    model.decode_batch_launch([0, 1, 2, 3])
    assert lib.dtk_set_guidance(ctx, 0, 1, 2.0) == -3 and lib.dtk_set_guidance(ctx, 0, -1, 1.0) == -3       # a step is in flight
    t = model.decode_batch_wait()
    assert t[0] == t[1] and t[2] == t[3] and t[0] >= 0 and t[2] >= 0
    model.decode_batch_launch([2, 3])                                                    # one whole pair alone
    t = model.decode_batch_wait()
    assert t[2] == t[3] and t[0] == -1
    model.set_guidance(None, 0, None)
    assert model.guidance(0) is None and model.guidance(3)["partner"] == 2
    model.set_guidance(1.0, 3, 2)                                                        # scale 1 dissolves
    assert model.guidance(3) is None and model.guidance(2) is None
    model.set_guidance(None, 1, None)                                                    # heads no pair: nothing to do
    model.decode_batch_launch([0])                                                       # and a single slot decodes again
    assert model.decode_batch_wait()[0] >= 0


# ------------------------------------------------------------------------------------------ generate(guidance_scale=...)
class _Tokens:
    def __init__(self):
        self.prompt, self.tokens, self.ended = None, [], False

    def put(self, value):
        if self.prompt is None:
            self.prompt = value.reshape(-1).tolist()
        else:
            self.tokens += value.reshape(-1).tolist()

    def end(self):
        self.ended = True


def test_generate_with_guidance(mv):
    model, proc = mv
    ids, px, px2 = _prompts(proc)
    T, N = int(ids.numel()), 16
    cfg = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=7)
    GEN = dict(input_ids=ids[None], pixel_values=px, guidance_scale=G, negative_pixel_values=px2, max_new_tokens=N, return_logprobs=True,
               bad_words_ids=[[IMG]], eos_token_id=-1, **cfg)
    sink = _Tokens()
    a = model.generate(streamer=sink, **GEN)
    b = model.generate(**GEN)
    new = a.sequences[0, T:].tolist()
    assert len(new) == N and torch.equal(a.sequences, b.sequences)
    assert a.logprobs.numpy().tobytes() == b.logprobs.numpy().tobytes() and a.sample_logprobs.numpy().tobytes() == b.sample_logprobs.numpy().tobytes()
    assert sink.prompt == ids.tolist() and sink.tokens == new and sink.ended
    assert model.guidance(0) is None and model.guidance(1) is None
    hand, bits, _ = _pair_by_hand(model, 0, 1, ids, px, px2, cfg, steps=N)
    assert hand == new and b"".join(bits) == a.logprobs.numpy().tobytes()
    # with the alternatives: the same tokens, the records of the guided distribution
    top = model.generate(top_logprobs=4, **GEN)
    assert torch.equal(top.sequences, a.sequences) and top.top_ids.shape == (1, N, 4)
    assert model.top_logprobs_enabled == 0
    # a presence penalty and a logit bias under guidance act on the mixed row
    bias = {new[0]: -4.0, new[1]: 2.5, 41: 1.0}
    shaped = model.generate(presence_penalty=0.7, logit_bias=bias, **GEN).sequences[0, T:].tolist()
    hand2, _, _ = _pair_by_hand(model, 0, 1, ids, px, px2, cfg, steps=N, pp=0.7, pairs=bias)
    assert shaped == hand2 and shaped != new
    assert int(model.logit_bias_table(slot=1).count_nonzero()) == 0                      # the unconditional slot stayed neutral
    # afterwards an unguided slot decodes what a fresh model's slot decodes
    def plain(m):
        m.set_sampling(slot=0, bad_ids=[IMG], **cfg)
        m.prefill(ids, px, slot=0)
        out = []
        for n in range(8):
            m.decode_batch_launch([0])
            out.append(m.decode_batch_wait()[0])
        return out
    fresh, _ = _load(5)
    assert plain(model) == plain(fresh)
    del fresh
    gc.collect()
    # unguided generate() is what it was, and the refusals come before anything runs
    unguided = model.generate(**{**GEN, "guidance_scale": None}).sequences
    assert torch.equal(unguided, model.generate(**{**GEN, "guidance_scale": 1.0}).sequences) and not torch.equal(unguided, a.sequences)
    with pytest.raises(ValueError, match="guidance_scale"):
        model.generate(**{**GEN, "guidance_scale": 101.0})
    print(f"worst |L - L64| of the op-level rows: {WORST['lse']:.3g}")


def test_pipeline_samples_with_guidance_on_a_tiny_adapter_model():
    """image prompts against the default white canvas, text prompts against another text: sample() returns a document, guided and
    repeatable, and the pair is gone afterwards"""
    from detikzify_amd.infer import DetikzifyPipeline, SyntheticTikzDocument
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny-v2", synthetic=4321, batch_slots=5, adapter=True, cross_attn_every_n_layers=2)
    pipe = DetikzifyPipeline(model, proc, metric="model", document_class=SyntheticTikzDocument, max_length=12 + 40, compile_timeout=None)
    image = sketch_image(4, 84)
    kw = dict(do_sample=True, seed=3, temperature=0.8)
    plain = pipe.sample(image, **kw)
    doc = pipe.sample(image, guidance_scale=1.5, **kw)
    assert isinstance(doc, SyntheticTikzDocument) and doc.code == pipe.sample(image, guidance_scale=1.5, **kw).code
    tdoc = pipe.sample(text="a red circle", guidance_scale=1.5, negative_text="a blue square", **kw)
    assert isinstance(tdoc, SyntheticTikzDocument) and tdoc.code == pipe.sample(text="a red circle", guidance_scale=1.5, negative_text="a blue square", **kw).code
    both = pipe.sample(image, text="a red circle", guidance_scale=1.5, negative_text="a blue square", negative_image=sketch_image(5, 84), **kw)
    assert isinstance(both, SyntheticTikzDocument)
    with pytest.raises(ValueError, match="negative_text"):
        pipe.sample(text="a red circle", guidance_scale=1.5, **kw)
    assert model.guidance(0) is None and pipe.sample(image, **kw).code == plain.code
    print(f"plain {len(plain.code)} chars, guided {len(doc.code)} / {len(tdoc.code)} chars; guided == plain: {doc.code == plain.code}")
    del pipe, model
    gc.collect()


def test_generate_needs_slots():
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny", synthetic=1234)
    ids, px, px2 = _prompts(proc)
    with pytest.raises(ValueError, match="batch_slots"):
        model.generate(input_ids=ids[None], pixel_values=px, guidance_scale=2.0, negative_pixel_values=px2, max_new_tokens=4)
    assert model.lib.dtk_set_guidance(model._ctx, 0, 1, 2.0) == -1
    del model
    gc.collect()
