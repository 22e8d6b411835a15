"""Packed candidate scoring on the MI355X (dtk_score_packed / model.score_candidates / DetikzifyPipeline.score_candidates): the
segmented attention kernel alone against a float64 masked softmax and its exact no-leak property, one candidate == score() bit for
bit, no leak through the whole model, the envelope of the CPU oracle (toy with an image, 2-layer real-width ds-7b), the context's
state afterwards, several passes, refusals, the pipeline."""
from __future__ import annotations

import ctypes as C
import gc

import numpy as np
import pytest
import torch

from oracle.model import DetikzifyOracle
from oracle.ops import bits_to_f32, f32_to_bits, rb
from tests.fullsize import weights_from_device
from tests.helpers import ENVELOPE, SLACK_LOGITS, TINY_CFG, envelope_ratio, rel_l2, sketch_image, top2_gap_ulps

pytestmark = pytest.mark.gpu


def _load(name, seed, **kw):
    from detikzify_amd.model import load
    return load(name, synthetic=seed, **kw)


@pytest.fixture(scope="module")
def tiny():
    return _load("detikzify-tiny", 1234)


@pytest.fixture(scope="module")
def tiny_v2():
    return _load("detikzify-tiny-v2", 4321)


@pytest.fixture(scope="module")
def tiny_tl():
    return _load("detikzify-tiny-tl", 77)


def _tokens(vocab, image_token_id, n, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab - 1, (n + 8,), generator=g)
    return ids[ids != image_token_id][:n].contiguous()


def _prompt(model, proc, image_seed=0, size=96):
    enc = proc(images=sketch_image(image_seed, size), return_tensors="pt")
    return enc.input_ids[0].to(torch.int64), enc.pixel_values


def _same(a, b):
    return torch.equal(a.logprobs, b.logprobs) and torch.equal(a.argmax, b.argmax) and torch.equal(a.lse, b.lse)


# ------------------------------------------------------------------------------------------ 1. the attention kernel alone
def _layout(shared, lens):
    """(seg_begin, kv_row) of the packed rows: `shared` prompt rows, then the segments"""
    begin, row = list([0] * shared), list(range(shared))
    r = shared
    for n in lens:
        begin += [r] * n
        row += list(range(r, r + n))
        r += n
    return np.asarray(begin, dtype=np.int32), np.asarray(row, dtype=np.int32)


def _masked_attention_f64(q, k, v, shared, begin, row):
    """softmax over the visible keys only, float64: query t sees key j iff j <= row[t] and (j < shared or j >= begin[t])"""
    j = torch.arange(k.shape[1])[None, :]
    b, r = torch.from_numpy(begin).long()[:, None], torch.from_numpy(row).long()[:, None]
    vis = (j <= r) & ((j < shared) | (j >= b))
    s = torch.einsum("htd,hjd->htj", q.double(), k.double()) * q.shape[-1] ** -0.5
    s = s.masked_fill(~vis[None], float("-inf"))
    return torch.einsum("htj,hjd->htd", torch.softmax(s, dim=-1), v.double())


def _ulp_report(got_bits, ref):
    """max difference in bf16 ulps of the reference (floored at 1 % of the tensor's largest magnitude) and rel-L2: the measure of
    test_op_attention"""
    got = bits_to_f32(got_bits).reshape(-1)
    ref = rb(torch.as_tensor(ref, dtype=torch.float32)).reshape(-1)
    ulp = torch.clamp(ref.abs(), min=1e-2 * float(ref.abs().max()) + 1e-30) * 2.0 ** -7
    return float(((got - ref).abs() / ulp).max()), rel_l2(got, ref)


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("shared,lens", [(0, [1, 1, 5]), (70, [3, 64, 1, 130, 17]), (128, [64, 64]), (10, [200, 200])])
def test_op_attention_seg(tiny, hd, shared, lens):
    """dtk_op_attention_seg with every packed row as a query (Tq = Tk): against the float64 masked softmax at test_op_attention's
    bar; then K and V of all OTHER segments are replaced by other random values and one segment's output must keep its bits — a
    masked key's value never matters, only the layout does."""
    model, _ = tiny
    H, T = 2, shared + sum(lens)
    begin, row = _layout(shared, lens)
    g = torch.Generator().manual_seed(hd + shared + len(lens))
    q, k, v = (rb(torch.randn(H, T, hd, generator=g)) for _ in range(3))
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def run(k_, v_):
        out = np.empty((H, T, hd), dtype=np.uint16)
        model._check(model.lib.dtk_op_attention_seg(model._ctx, p(f32_to_bits(q)), p(f32_to_bits(k_)), p(f32_to_bits(v_)), H, T, T, hd,
                                                    shared, p(begin), p(row), p(out)), "dtk_op_attention_seg")
        return out
    out = run(k, v)
    ulps, rl2 = _ulp_report(out, _masked_attention_f64(q, k, v, shared, begin, row))
    print(f"attention_seg hd{hd} shared {shared} segments {lens}: max_ulp {ulps:.2f} rel_l2 {rl2:.2e}")
    assert rl2 < 2e-3 and ulps <= 4.01
    keep = len(lens) // 2                                     # the segment whose rows must not move
    lo = shared + sum(lens[:keep])
    hi = lo + lens[keep]
    others = torch.ones(T, dtype=torch.bool)
    others[:shared] = False
    others[lo:hi] = False
    k2, v2 = k.clone(), v.clone()
    k2[:, others] = rb(torch.randn(H, int(others.sum()), hd, generator=g) * 3)
    v2[:, others] = rb(torch.randn(H, int(others.sum()), hd, generator=g) * 3)
    out2 = run(k2, v2)
    assert np.array_equal(out2[:, lo:hi], out[:, lo:hi]) and np.array_equal(out2[:, :shared], out[:, :shared])
    if len(lens) > 1:
        assert not np.array_equal(out2, out)                  # the other segments did see their new keys


# ------------------------------------------------------------------------------------------ 2. one candidate is score()
@pytest.mark.parametrize("which", ["tiny", "tiny_v2", "tiny_tl"])
def test_one_candidate_is_score_bit_for_bit(which, request):
    model, proc = request.getfixturevalue(which)
    prefix, px = _prompt(model, proc)
    cand = _tokens(model.config.vocab, int(model.config.image_token_id), 40, 11)
    P = prefix.numel()
    want = model.score(torch.cat([prefix, cand]), px, first=P, reuse=False)
    got = model.score_candidates(prefix, [cand], px, reuse=False)
    assert len(got) == 1 and got[0].first == P and got[0].logprobs.numel() == 40
    assert got[0].logprobs.dtype == torch.float32 and got[0].argmax.dtype == torch.int64
    assert _same(got[0], want)


# ------------------------------------------------------------------------------------------ 3. no leak through the whole model
@pytest.mark.parametrize("which", ["tiny", "tiny_v2"])
def test_other_candidates_do_not_leak_into_a_candidate(which, request):
    model, proc = request.getfixturevalue(which)
    prefix, px = _prompt(model, proc, image_seed=2)
    V, img = model.config.vocab, int(model.config.image_token_id)
    lens = (1, 2, 17, 40, 9)
    a = [_tokens(V, img, n, 20 + i) for i, n in enumerate(lens)]
    b = [_tokens(V, img, n, 40 + i) for i, n in enumerate(lens)]
    b[2] = a[2]
    first = model.score_candidates(prefix, a, px, reuse=False)
    again = model.score_candidates(prefix, a, px, reuse=False)
    other = model.score_candidates(prefix, b, px, reuse=False)
    assert [o.logprobs.numel() for o in first] == list(lens)
    assert all(_same(x, y) for x, y in zip(first, again))
    assert _same(first[2], other[2])
    assert not torch.equal(first[3].logprobs, other[3].logprobs)
    # every candidate alone, in a pass of its own
    alone = model.score_candidates(prefix, [a[3]], px, reuse=False)[0]
    print(f"{which}: candidate 3 packed with four others vs alone: rel_l2 {rel_l2(first[3].logprobs, alone.logprobs):.2e}")


# ------------------------------------------------------------------------------------------ 4. against the CPU oracle
def _oracle_candidates(oracle, prefix, px, cands):
    """[(log-probabilities float64, logits rows fp32)] per candidate: the prompt prefilled once, every candidate teacher-forced behind it"""
    last = oracle.prefill(prefix, px)
    snap = oracle.snapshot()
    out = []
    for c in cands:
        oracle.restore(snap)
        rows = [last.float()]
        if c.numel() > 1:
            rows += [r.float() for r in oracle.extend(c[:-1].tolist())]
        logits = torch.stack(rows)
        out.append((torch.log_softmax(logits.double(), dim=-1).gather(1, c[:, None])[:, 0], logits))
    return out


def _check_against_oracles(tag, model, cfg, w, prefix, px, cands, outs, sequential=None):
    o16 = _oracle_candidates(DetikzifyOracle(cfg, w, precision="bf16"), prefix, px, cands)
    o32 = _oracle_candidates(DetikzifyOracle(cfg, w, precision="fp32"), prefix, px, cands)
    near_total = rows_total = 0
    for i, (out, (lp16, _), (lp32, rows32)) in enumerate(zip(outs, o16, o32)):
        e_dev, e_orc = rel_l2(out.logprobs, lp32), rel_l2(lp16, lp32)
        near = [top2_gap_ulps(r, [], [], False) <= 2.0 for r in rows32]
        near_total, rows_total = near_total + sum(near), rows_total + len(near)
        line = (f"{tag} candidate {i} ({out.logprobs.numel()} tokens): vs fp32 oracle: device {e_dev:.2e}, bf16 oracle {e_orc:.2e}, "
                f"ratio to the envelope {envelope_ratio(e_dev, e_orc):.2f}; {sum(near)} near-tie rows")
        if sequential is not None:
            line += f"; rel_l2 to the sequential score() {rel_l2(out.logprobs, sequential[i].logprobs):.2e}"
        print(line)
        assert e_dev <= ENVELOPE * e_orc + SLACK_LOGITS, (tag, i, e_dev, e_orc)
        for k, (a, r) in enumerate(zip(out.argmax.tolist(), rows32)):
            if not near[k]:
                assert a == int(torch.argmax(r)), (tag, i, k, a, int(torch.argmax(r)))
    print(f"{tag}: {near_total} of {rows_total} fp32-oracle rows are near-ties (top-2 gap within 2 bf16 ulps)")
    assert 4 * near_total <= rows_total, (tag, near_total, rows_total)


def test_toy_with_an_image_is_inside_the_envelope_of_the_cpu_oracle():
    model, proc = _load("detikzify-tiny", 1234, max_positions=512)
    try:
        cfg = dict(TINY_CFG, max_positions=512)
        w = weights_from_device(model, cfg)
        prefix, px = _prompt(model, proc)
        cands = [_tokens(cfg["vocab"], cfg["image_token_id"], n, 60 + i) for i, n in enumerate((1, 2, 63, 64, 65, 130))]
        sequential = [model.score(torch.cat([prefix, c]), px, first=prefix.numel(), reuse=True) for c in cands]
        outs = model.score_candidates(prefix, cands, px, reuse=False)
        _check_against_oracles("toy v1, image", model, cfg, w, prefix, px[0], cands, outs, sequential)
    finally:
        del model
        gc.collect()


def _two_layer(name, max_positions=1024, seed=99):
    from detikzify_amd.model.config import preset
    from detikzify_amd.model.modeling import DetikzifyForCausalLM
    cfg = preset(name)
    cfg.layers, cfg.max_positions = 2, max_positions
    model = DetikzifyForCausalLM(cfg, 0)
    model.fill_synthetic(seed)
    return model


def test_real_width_is_inside_the_envelope_of_the_cpu_oracle():
    """2-layer ds-7b at the real d and V, a 40-token text prompt and candidates of 1, 2, 63, 64, 65 and 300 tokens: 534 rows in one
    pass (the one-launch sliced GEMMs and k_gemm_g3's log-softmax epilogue), segments on both sides of a key-tile edge."""
    model = _two_layer("detikzify-ds-7b")
    try:
        cfg = model.config.oracle_dict()
        w = weights_from_device(model, cfg, skip_prefix="vision_model.")
        prefix = _tokens(cfg["vocab"], cfg["image_token_id"], 40, 5)
        cands = [_tokens(cfg["vocab"], cfg["image_token_id"], n, 70 + i) for i, n in enumerate((1, 2, 63, 64, 65, 300))]
        sequential = [model.score(torch.cat([prefix, c]), None, first=40, reuse=True) for c in cands]
        outs = model.score_candidates(prefix, cands, None, reuse=False)
        _check_against_oracles("ds-7b 2 layers", model, cfg, w, prefix, None, cands, outs, sequential)
    finally:
        del model
        gc.collect()


# ------------------------------------------------------------------------------------------ 5. state afterwards
def test_context_after_a_packed_call(tiny):
    from detikzify_amd._lib import DtkError
    model, proc = tiny
    prefix, px = _prompt(model, proc, image_seed=4)
    V, img = model.config.vocab, int(model.config.image_token_id)
    cands = [_tokens(V, img, n, 80 + i) for i, n in enumerate((7, 12, 3))]
    x = _tokens(V, img, 9, 90)
    full = torch.cat([prefix, x])
    cold = model.prefill(full, px, return_logits=True, reuse=False)
    model.score_candidates(prefix, cands, px, reuse=False)
    assert model.context_len() == prefix.numel() - 1
    with pytest.raises(DtkError):
        model.decode_launch()
    before = model.stats()
    warm = model.prefill(full, px, return_logits=True, reuse=True)
    after = model.stats()
    assert torch.equal(warm, cold)
    assert after["prefill_tokens"] - before["prefill_tokens"] == x.numel() + 1        # position P-1 and the tail: the prompt was reused
    assert after["vit_images"] == before["vit_images"]
    model.set_sampling(do_sample=False)
    model.decode_launch()
    model.decode_wait()                                        # and the context decodes again


# ------------------------------------------------------------------------------------------ 6. several passes
def test_candidates_that_need_three_passes(tiny):
    _, proc0 = tiny
    P = _prompt(None, proc0)[0].numel()
    L = 30
    model, proc = _load("detikzify-tiny", 1234, max_positions=P - 1 + 2 * L + L // 2)
    try:
        cfg = dict(TINY_CFG, max_positions=model.config.max_positions)
        w = weights_from_device(model, cfg)
        prefix, px = _prompt(model, proc)
        assert prefix.numel() == P
        cands = [_tokens(cfg["vocab"], cfg["image_token_id"], L - (i % 3), 100 + i) for i in range(6)]
        from detikzify_amd.model.packing import plan_packed_passes
        assert len(plan_packed_passes(P, [c.numel() for c in cands], model.config.max_positions)) == 3
        model.score_candidates(prefix, cands[:1], px, reuse=False)              # the image is encoded here
        s0 = model.stats()
        outs = model.score_candidates(prefix, cands, px, reuse=True)
        s1 = model.stats()
        assert s1["vit_images"] == s0["vit_images"]                            # no pass of the three encoded the image again
        # first pass: position P-1's rows and the candidates only (the prompt is cached); the others the same
        assert s1["prefill_tokens"] - s0["prefill_tokens"] == sum(c.numel() for c in cands)
        assert [o.logprobs.numel() for o in outs] == [c.numel() for c in cands]
        cold = model.score_candidates(prefix, cands, px, reuse=False)
        s2 = model.stats()
        assert s2["vit_images"] == s1["vit_images"] + 1                        # reuse=False: the first pass encodes, the later two do not
        assert all(_same(a, b) for a, b in zip(outs, cold))
        _check_against_oracles("toy v1, three passes", model, cfg, w, prefix, px[0], cands, outs)
    finally:
        del model
        gc.collect()


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_happen_before_any_launch(tiny):
    """every refusal leaves the context as it was: prefill_tokens and context_len unchanged, and a following score() that reuses the
    cache computes its tail only (a wiped cache would recompute the probe's head) and gives the same bits"""
    from detikzify_amd import _lib
    model, proc = tiny
    V, Tmax = TINY_CFG["vocab"], TINY_CFG["max_positions"]
    prefix = torch.tensor([5, 6, 7, 8], dtype=torch.int64)
    probe = torch.tensor([5, 6, 7, 8, 9, 10], dtype=torch.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(cand_ids, cand_len, n=None, pfx=prefix):
        ids = np.asarray(cand_ids, dtype=np.int64)
        lens = np.asarray(cand_len, dtype=np.int32)
        out = np.empty(max(ids.size, 1), dtype=np.float32)
        rc = model.lib.dtk_score_packed(model._ctx, p(pfx.numpy()), pfx.numel(), None, C.c_uint64(0), C.c_uint32(0),
                                        p(ids), p(lens), len(cand_len) if n is None else n, p(out), None, None)
        return rc, (model.lib.dtk_last_error(model._ctx) or b"").decode(), out

    def fresh():
        """the probe scored and cached; (its result, prefill_tokens)"""
        return model.score(probe, None, first=5, reuse=False), model.stats()["prefill_tokens"]

    def untouched(good, tokens_before):
        assert model.stats()["prefill_tokens"] == tokens_before
        assert model.context_len() == probe.numel()
        again = model.score(probe, None, first=5, reuse=True)
        assert model.stats()["prefill_tokens"] - tokens_before == 2          # positions 4 and 5: the cached head was still there
        assert _same(again, good)

    room = Tmax - (prefix.numel() - 1)
    one = prefix[:1]
    cases = [("capacity + 1", prefix, [7] * (room + 1), [room + 1], None, -4, "max_positions"),        # DTK_ERR_RANGE
             ("capacity + 1 behind a one-token prompt", one, [7] * (Tmax + 1), [Tmax + 1], None, -4, "max_positions"),
             ("N = 0", prefix, [7], [1], 0, -1, "N >= 1"),
             ("empty candidate", prefix, [7, 8], [2, 0], None, -1, "len >= 1"),
             ("id >= V", prefix, [7, V], [2], None, -1, "outside")]
    for tag, pfx, ids, lens, n, code, msg in cases:
        good, t0 = fresh()
        rc, text, _ = call(ids, lens, n, pfx)
        print(f"{tag}: rc {rc}: {text}")
        assert rc == code and msg in text, (tag, rc, text)
        untouched(good, t0)
    # the same through Python
    with pytest.raises(ValueError, match="max_positions"):
        model.score_candidates(prefix, [torch.full((room + 1,), 7)])
    with pytest.raises(ValueError, match="empty"):
        model.score_candidates(prefix, [torch.tensor([7, 8]), torch.tensor([], dtype=torch.int64)])
    with pytest.raises(ValueError):
        model.score_candidates(prefix, [])
    with pytest.raises(_lib.DtkError, match="outside"):
        model.score_candidates(prefix, [torch.tensor([7, V])])
    # exactly at capacity is taken; behind a one-token prompt that is max_positions scored rows, every one with its record
    rc, text, _ = call([7] * room, [room])
    assert rc == 0, text
    full = _tokens(V, int(model.config.image_token_id), Tmax, 123)
    rc, text, lp = call(full.tolist(), [Tmax], pfx=one)
    assert rc == 0, text
    want = model.score(torch.cat([one, full[:-1]]), None, first=1, reuse=False)      # the same rows but the last, as dtk_score holds them
    assert np.array_equal(lp[:Tmax - 1], want.logprobs.numpy()) and np.isfinite(lp[Tmax - 1]) and lp[Tmax - 1] < 0
    # attn_impl = 1: the VALU attention kernel has no segmented form
    model.set_option("attn_impl", 1)
    try:
        good, t0 = fresh()
        with pytest.raises(_lib.DtkError, match="attn_impl"):
            model.score_candidates(prefix, [torch.tensor([9, 10])])
        untouched(good, t0)
    finally:
        model.set_option("attn_impl", 0)


def test_image_placeholder_inside_a_candidate(tiny):
    """with an image in use the placeholders must lie in the prompt (refused, nothing launched); without one the id is a token like
    any other and the result is score()'s"""
    model, proc = tiny
    img = int(model.config.image_token_id)
    prefix, px = _prompt(model, proc, image_seed=6)
    cand = torch.tensor([9, img, 11], dtype=torch.int64)
    t0 = model.stats()["prefill_tokens"]
    with pytest.raises(ValueError, match="image patch tokens"):
        model.score_candidates(prefix, [cand], px, reuse=False)
    assert model.stats()["prefill_tokens"] == t0
    text = torch.tensor([5, 6, 7, 8], dtype=torch.int64)
    got = model.score_candidates(text, [cand], None, reuse=False)[0]
    assert _same(got, model.score(torch.cat([text, cand]), None, first=4, reuse=False))


# ------------------------------------------------------------------------------------------ 7b. text conditioning
def test_text_conditioned_candidates_are_score_bit_for_bit():
    """dtk_score_packed_text on an adapter-loaded toy model: one candidate equals score(adapter_input_ids=...) bit for bit, with an
    image and with the adapter's dummy input; another second candidate leaves the first one's bits alone; the text matters"""
    model, proc = _load("detikzify-tiny-v2", 4321, adapter=True, cross_attn_every_n_layers=2)
    try:
        V, img = model.config.vocab, int(model.config.image_token_id)
        text = torch.randint(0, 300, (40,), generator=torch.Generator().manual_seed(3), dtype=torch.int64)
        enc = proc(images=sketch_image(1, 84), return_tensors="pt")
        prefix, px = enc.input_ids[0].to(torch.int64), enc.pixel_values
        a, b = _tokens(V, img, 24, 4), _tokens(V, img, 9, 6)
        P = prefix.numel()
        for tag, pixels in (("text + image", px), ("text only", None)):
            want = model.score(torch.cat([prefix, a]), pixels, first=P, adapter_input_ids=text, reuse=False)
            got = model.score_candidates(prefix, [a], pixels, adapter_input_ids=text, reuse=False)
            assert len(got) == 1 and _same(got[0], want), tag
            two = model.score_candidates(prefix, [a, b], pixels, adapter_input_ids=text, reuse=True)
            swapped = model.score_candidates(prefix, [a, torch.flip(b, [0])], pixels, adapter_input_ids=text, reuse=True)
            assert two[1].logprobs.numel() == 9 and _same(two[0], swapped[0]), tag
        plain = model.score_candidates(prefix, [a], px, reuse=False)[0]
        assert not torch.equal(plain.logprobs, got[0].logprobs)
    finally:
        del model
        gc.collect()


# ------------------------------------------------------------------------------------------ 8. pipeline
def test_pipeline_score_candidates(tiny):
    from detikzify_amd.infer import DetikzifyPipeline
    model, proc = tiny
    pipe = DetikzifyPipeline(model, proc, metric="fast", compile_timeout=None)
    image = sketch_image(5, 96)
    codes = ["\\draw (0,0) -- (1,1);\n\\node at (2,2) {x};\n", "\\fill (0,0) circle (1);\n", "\\draw (0,0) rectangle (3,2);\n\\draw (1,1) -- (2,2);\n"]
    tok = proc.tokenizer
    got = pipe.score_candidates(image, codes=codes)
    assert len(got) == 3
    for code, (total, per_token) in zip(codes, got):
        assert len(per_token) == len(tok.encode(code, add_special_tokens=False)) + 1
        assert total == pytest.approx(sum(per_token), rel=1e-6)
        want, _ = pipe.score(image, code=code)
        print(f"pipeline: packed {total:.4f}, score() {want:.4f}")
        assert abs(total - want) <= 1e-2 * abs(want)
