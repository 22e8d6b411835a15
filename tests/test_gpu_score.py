"""Teacher-forced scoring on the MI355X (dtk_score / model.score / model.forward(labels=...) / DetikzifyPipeline.score): the
log-softmax lm_head kernels alone, against the reference model's own all-position logits (goldens), inside the parity envelope of
the CPU oracle (toy size, 2-layer real-width models, full-size ds-1.3b and v2-8b through tests/fullsize.py), their exact
invariances, the path users had before (one prefill per position), the adapter, errors, the pipeline."""
from __future__ import annotations

import ctypes as C
import gc
import time

import numpy as np
import pytest
import torch

from oracle.model import DetikzifyOracle
from oracle.ops import bits_to_f32, f32_to_bits, rb
from oracle.synth import tensor_specs
from tests.fullsize import weights_from_device
from tests.helpers import (ENVELOPE, SLACK_LOGITS, TINY, TINY_CFG, TINY_V2, TINY_V2_CFG, envelope_ratio, rel_l2, sketch_image,
                           top2_gap_ulps)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    from detikzify_amd.model import load
    return load("detikzify-tiny", synthetic=1234)


@pytest.fixture(scope="module")
def tiny_v2():
    from detikzify_amd.model import load
    return load("detikzify-tiny-v2", synthetic=4321)


def _oracle_logprobs(oracle, ids, px, first, vit_feats=None):
    """(log-probabilities of ids[first:], the rows' logits) by one oracle: prefill of ids[:first], then one teacher-forced pass"""
    last = oracle.prefill(ids[:first], px, vit_feats=vit_feats) if vit_feats is not None else oracle.prefill(ids[:first], px)
    rows = [last]
    if ids.numel() - first > 1:
        rows += list(oracle.extend(ids[first:-1].tolist()))
    logits = torch.stack([r.float() for r in rows])
    lp = torch.log_softmax(logits.double(), dim=-1).gather(1, ids[first:, None])[:, 0]
    return lp, logits


def _envelope(tag, dev_lp, lp16, lp32):
    e_dev, e_orc = rel_l2(dev_lp, lp32), rel_l2(lp16, lp32)
    ratio = envelope_ratio(e_dev, e_orc)
    print(f"{tag}: log-probabilities vs fp32 oracle: device {e_dev:.2e}, bf16 oracle {e_orc:.2e}, ratio to the envelope {ratio:.2f}")
    assert e_dev <= ENVELOPE * e_orc + SLACK_LOGITS, (tag, e_dev, e_orc)
    return ratio


def _argmax_agrees(tag, dev_argmax, ref_logits):
    """device argmax == the reference's, except where the REFERENCE's own top two are within 2 bf16 ulps; at most a quarter of the
    positions may be such near-ties"""
    near = [top2_gap_ulps(r, [], [], False) <= 2.0 for r in ref_logits]
    print(f"{tag}: {sum(near)} of {len(near)} reference rows are near-ties (top-2 gap within 2 bf16 ulps)")
    assert 4 * sum(near) <= len(near), (tag, sum(near), len(near))
    for k, (a, r) in enumerate(zip(dev_argmax.tolist(), ref_logits)):
        if not near[k]:
            assert a == int(torch.argmax(r)), (tag, k, a, int(torch.argmax(r)))


# ------------------------------------------------------------------------------------------ the kernel pair alone
@pytest.mark.parametrize("M,N,K,wt", [(37, 1000, 64, 0), (130, 515, 304, 0), (64, 128, 64, 0),          # k_gemm_mfma<64, 128>: ragged N, ragged M
                                      (300, 16424, 128, 0), (70, 16424, 192, 1), (257, 16512, 256, 1),    # k_gemm_g3 (ceil(N / 128) >= 128): tall / wide tile, W stage from tiles
                                      (70, 16424, 200, 1), (300, 16424, 200, 0), (130, 16424, 136, 1)])   # ... with a ragged K tail (K % 64 != 0: the register-staged last stage, then the records parked over stage 0)
def test_op_score_against_the_gemm_kernels_own_logits(tiny, M, N, K, wt):
    """dtk_op_score against log_softmax (float64) of what dtk_op_gemm stores for the same operands: every GEMM kernel here runs the
    same k order per output, so z is the same bf16 value and only exp / log / the fp32 sums differ: |d logprob|, |d lse| <= 2e-5
    (a few fp32 ulps of |lse| ~ 10 and of the sum of <= 16.5 k terms); argmax (lowest index on ties) and z[argmax] exact."""
    from detikzify_amd import _lib
    model, _ = tiny
    g = torch.Generator().manual_seed(M + N + K)
    A = rb(torch.randn(M, K, generator=g)); W = rb(torch.randn(N, K, generator=g) * 0.3)
    W[N // 3] = W[N // 3 + 5]                      # an exact tie somewhere: the lower index must win wherever it is the maximum
    tg = torch.randint(0, N, (M,), generator=g, dtype=torch.int32)
    tg[0], tg[-1] = 0, N - 1
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    Ab, Wb, Tb = f32_to_bits(A), f32_to_bits(W), tg.numpy()
    z = np.empty((M, N), dtype=np.uint16)
    model._check(model.lib.dtk_op_gemm(model._ctx, p(Ab), p(Wb), None, None, M, N, K, 0, p(z)), "dtk_op_gemm")
    zf = bits_to_f32(z)
    lp, lse, am, zm = (np.empty(M, dtype=np.float32), np.empty(M, dtype=np.float32), np.empty(M, dtype=np.int32), np.empty(M, dtype=np.float32))
    model._check(model.lib.dtk_op_score(model._ctx, p(Ab), p(Wb), p(Tb), M, N, K, _lib.DTK_GEMM_WT if wt else 0, p(lp), p(lse), p(am), p(zm)),
                 "dtk_op_score")
    ref_lse = torch.logsumexp(zf.double(), dim=-1)
    ref_lp = zf.double().gather(1, tg.long()[:, None])[:, 0] - ref_lse
    d_lp, d_lse = float((torch.from_numpy(lp).double() - ref_lp).abs().max()), float((torch.from_numpy(lse).double() - ref_lse).abs().max())
    print(f"op_score {M}x{N}x{K} wt={wt}: max |d logprob| {d_lp:.2e}, max |d lse| {d_lse:.2e}")
    lowest = torch.where(zf == zf.max(dim=-1, keepdim=True)[0], torch.arange(N)[None, :], N).min(dim=-1)[0]
    assert torch.equal(torch.from_numpy(am).long(), lowest)
    assert torch.equal(torch.from_numpy(zm), zf.max(dim=-1)[0])
    assert d_lp <= 2e-5 and d_lse <= 2e-5
    # a row's outputs do not depend on M or on its neighbours: the first rows alone give the same bits
    M2 = max(1, M // 3)
    lp2, am2 = np.empty(M2, dtype=np.float32), np.empty(M2, dtype=np.int32)
    model._check(model.lib.dtk_op_score(model._ctx, p(Ab), p(Wb), p(Tb), M2, N, K, 0, p(lp2), None, p(am2), None), "dtk_op_score")
    assert np.array_equal(lp2, lp[:M2]) and np.array_equal(am2, am[:M2])


# ------------------------------------------------------------------------------------------ the reference's own model code
@pytest.mark.parametrize("which", ["v1", "v2"])
def test_score_against_the_reference_models_own_logits(which, tiny, tiny_v2, golden_dir):
    """score(ids, pixels, first=1) against log_softmax of the reference model's fp32 logits of every position
    (tests/golden/reference_v{1,2}_tiny.npz: prefill_logits [15][V]); 1e-2 rel-L2 on the vector of
    log-probabilities, argmax equal outside the golden's own near-ties; forward(labels=ids).loss = torch's CrossEntropyLoss."""
    model = (tiny if which == "v1" else tiny_v2)[0]
    g = np.load(golden_dir / f"reference_{which}_tiny.npz")
    ids, px = torch.from_numpy(g["ids"]).to(torch.int64), torch.from_numpy(g["pixels"])
    logits = torch.from_numpy(g["prefill_logits"]).float()
    ref = torch.log_softmax(logits.double(), dim=-1)[:-1].gather(1, ids[1:, None])[:, 0]
    out = model.score(ids, px, first=1)
    assert out.logprobs.dtype == torch.float32 and out.argmax.dtype == torch.int64 and out.logprobs.numel() == ids.numel() - 1
    r = rel_l2(out.logprobs, ref)
    print(f"{which}: device log-probabilities vs the reference model's: rel_l2 {r:.2e}")
    assert r < 1e-2
    _argmax_agrees(which, out.argmax, logits[:-1])
    assert bool(torch.isfinite(out.lse).all()) and bool((out.logprobs <= 0).all())
    loss = model(input_ids=ids[None], pixel_values=px, labels=ids[None]).loss
    want = torch.nn.CrossEntropyLoss()(logits[:-1], ids[1:])
    print(f"{which}: forward(labels).loss {float(loss):.6f}, CrossEntropyLoss on the reference logits {float(want):.6f}")
    assert loss.dtype == torch.float32 and abs(float(loss) - float(want)) <= 1e-2 * abs(float(want))


# ------------------------------------------------------------------------------------------ envelope against the CPU oracle
def _two_layer(name, weight_format="bf16", max_positions=1024, seed=99):
    from detikzify_amd.model.config import preset
    from detikzify_amd.model.modeling import DetikzifyForCausalLM
    cfg = preset(name)
    cfg.layers, cfg.max_positions, cfg.weight_format = 2, max_positions, weight_format
    model = DetikzifyForCausalLM(cfg, 0)
    model.fill_synthetic(seed)
    return model


def _text_prompt(cfg, n, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, cfg["vocab"] - 1, (n + 8,), generator=g)
    return ids[ids != cfg["image_token_id"]][:n].contiguous()


def test_toy_score_is_inside_the_envelope_of_the_cpu_oracle(tiny):
    model, proc = tiny
    w = weights_from_device(model, TINY_CFG)
    enc = proc(images=sketch_image(0, 96), return_tensors="pt")
    g = torch.Generator().manual_seed(11)
    prog = torch.randint(3, TINY_CFG["vocab"] - 1, (40,), generator=g)
    ids, px = torch.cat([enc.input_ids[0], prog]), enc.pixel_values
    first = model.default_first(ids)
    assert first == enc.input_ids[0].numel() or int(ids[first - 1]) == TINY.image_token_id
    out = model.score(ids, px)
    assert out.first == first and out.logprobs.numel() == ids.numel() - first
    lp16, _ = _oracle_logprobs(DetikzifyOracle(TINY_CFG, w, precision="bf16"), ids, px[0], first)
    lp32, rows32 = _oracle_logprobs(DetikzifyOracle(TINY_CFG, w, precision="fp32"), ids, px[0], first)
    _envelope("toy v1, image + 40 tokens", out.logprobs, lp16, lp32)


@pytest.mark.parametrize("name,weight_format", [("detikzify-ds-7b", "bf16"), ("detikzify-v2-8b", "bf16"), ("detikzify-cl-7b", "fp8")])
def test_real_width_score_envelope_and_exact_properties(name, weight_format):
    """2-layer models at the real d and V (k_gemm_g3 with the log-softmax epilogue; fp8: the de-quantised lm_head), text prompts.
    Envelope on 300 rows; then the exact properties: a prefix of the same size class scores the same bits on the common positions, so
    does another `first`; scoring leaves the context as prefill does.  Size classes of the prefill's kernels: <= 128 rows, 129 .. 768,
    > 768; where a prefix falls into another class the hidden states differ by fp32 summation order, so the envelope is asserted
    there instead of equality."""
    model = _two_layer(name, weight_format)
    try:
        cfg = model.config.oracle_dict()
        w = weights_from_device(model, cfg, skip_prefix="vision_model.")
        ids = _text_prompt(cfg, 300, 5)
        out = model.score(ids, None, first=1)
        o16, o32 = DetikzifyOracle(cfg, w, precision="bf16"), DetikzifyOracle(cfg, w, precision="fp32")
        lp16, _ = _oracle_logprobs(o16, ids, None, 1)
        lp32, rows32 = _oracle_logprobs(o32, ids, None, 1)
        _envelope(f"{name} {weight_format} 2 layers, 300 rows", out.logprobs, lp16, lp32)
        near = sum(top2_gap_ulps(r, [], [], False) <= 2.0 for r in rows32)
        print(f"{name}: {near} of {len(rows32)} fp32-oracle rows are near-ties")
        # same size class (129 .. 768 rows): exact
        short = model.score(ids[:200], None, first=1)
        assert torch.equal(short.logprobs, out.logprobs[:199]) and torch.equal(short.argmax, out.argmax[:199]) and torch.equal(short.lse, out.lse[:199])
        late = model.score(ids, None, first=150)
        assert torch.equal(late.logprobs, out.logprobs[149:]) and torch.equal(late.argmax, out.argmax[149:])
        # <= 128 rows against its own prefix
        a, b = model.score(ids[:120], None, first=1), model.score(ids[:64], None, first=1)
        assert torch.equal(b.logprobs, a.logprobs[:63]) and torch.equal(b.argmax, a.argmax[:63])
        # another class (120 rows vs 300): envelope, not equality
        _envelope(f"{name}: 120-row prompt (another size class)", a.logprobs, lp16[:119], lp32[:119])
        # > 768 rows against its own prefix
        long_ids = _text_prompt(cfg, 900, 6)
        c, d = model.score(long_ids, None, first=1), model.score(long_ids[:800], None, first=1)
        assert torch.equal(d.logprobs, c.logprobs[:799]) and torch.equal(d.argmax, c.argmax[:799])
        # the context after score == the context after prefill: logits of the last row and 16 greedy tokens
        model.set_sampling(do_sample=False)
        model.score(ids, None, first=100)
        lg_s = model.get_logits()
        toks_s = []
        for _ in range(16):
            model.decode_launch(); toks_s.append(model.decode_wait())
        ref_lg = model.prefill(ids, None, return_logits=True)
        assert torch.equal(model.get_logits(), ref_lg) and torch.equal(lg_s, ref_lg)
        toks_p = []
        for _ in range(16):
            model.decode_launch(); toks_p.append(model.decode_wait())
        assert toks_s == toks_p
    finally:
        del model
        gc.collect()


@pytest.mark.parametrize("name", ["detikzify-ds-1.3b", "detikzify-v2-8b"])
def test_full_size_score_is_inside_the_envelope_of_the_cpu_oracle(name):
    """Full depth (24 / 32 layers of accumulated bf16 error under the log-softmax; ds-1.3b: d = 2048, V = 32 256) with the seed-1234
    weights: the image prefix of tests/fullsize.py's shared snapshot (both oracles prefilled once), then 48 program tokens
    teacher-forced by `oracle.extend` in one pass against ONE `score` call; ENVELOPE / SLACK_LOGITS of tests/helpers.py on the vector
    of log-probabilities, the ratio printed.  Prefix reuse on a second program must give the cold call's bits here too."""
    from detikzify_amd.model import load
    from tests.fullsize import host_side
    model, proc = load(name, synthetic=1234, max_positions=512)
    try:
        hs = host_side(model, proc, name, "bf16")
        cfg, _, o16, o32 = hs.oracles(model)
        g = torch.Generator().manual_seed(17)
        prog = torch.randint(3, cfg["vocab"] - 1, (56,), generator=g)
        prog = prog[prog != cfg["image_token_id"]][:48].contiguous()
        ids, first = torch.cat([hs.ids, prog]), hs.n_img
        assert model.default_first(ids) == first
        out = model.score(ids, hs.px)
        assert out.first == first and out.logprobs.numel() == prog.numel()

        def teacher_forced(oracle, last):
            rows = torch.stack([last.float()] + [r.float() for r in oracle.extend(prog[:-1].tolist())])
            return torch.log_softmax(rows.double(), dim=-1).gather(1, prog[:, None])[:, 0], rows
        lp16, _ = teacher_forced(o16, hs.ref)
        lp32, rows32 = teacher_forced(o32, hs.truth)
        _envelope(f"{name} full size, {first}-token image prefix + {prog.numel()} tokens", out.logprobs, lp16, lp32)
        near = [top2_gap_ulps(r, [], [], False) <= 2.0 for r in rows32]
        flips = sum(a != int(torch.argmax(r)) for a, r in zip(out.argmax.tolist(), rows32))
        print(f"{name}: {sum(near)} of {len(near)} fp32-oracle rows are near-ties; device argmax differs from the fp32 oracle's at {flips}")
        prog2 = torch.cat([prog[:5], torch.flip(prog[5:30], [0])])
        cold = model.score(torch.cat([hs.ids, prog2]), hs.px, reuse=False)
        model.score(ids, hs.px, reuse=True)
        warm = model.score(torch.cat([hs.ids, prog2]), hs.px, reuse=True)
        assert torch.equal(warm.logprobs, cold.logprobs) and torch.equal(warm.argmax, cold.argmax)
    finally:
        del model
        gc.collect()


def test_reuse_flags_score_a_second_program_like_a_cold_call(tiny):
    model, proc = tiny
    enc = proc(images=sketch_image(3, 96), return_tensors="pt")
    g = torch.Generator().manual_seed(2)
    p1, p2 = torch.randint(3, 500, (30,), generator=g), torch.randint(3, 500, (25,), generator=g)
    p2[:4] = p1[:4]                            # the programs share their first tokens: the reused prefix must stop before the scored rows
    px = enc.pixel_values
    cold = model.score(torch.cat([enc.input_ids[0], p2]), px, reuse=False)
    model.score(torch.cat([enc.input_ids[0], p1]), px, reuse=True)
    vit0 = model.stats()["vit_images"]
    warm = model.score(torch.cat([enc.input_ids[0], p2]), px, reuse=True)
    assert model.stats()["vit_images"] == vit0          # the image was not encoded again
    assert torch.equal(warm.logprobs, cold.logprobs) and torch.equal(warm.argmax, cold.argmax) and torch.equal(warm.lse, cold.lse)


# ------------------------------------------------------------------------------------------ the path users had before
def test_score_agrees_with_one_prefill_per_position():
    """8 positions of a 300-row prompt: log_softmax (float64, host) of prefill(ids[:t], return_logits=True) against score's value.
    Both are fp32 sums of the same products in another order (and another prefill size class for short t): each side is asserted
    inside the envelope of the CPU oracle; their largest difference is printed, not asserted."""
    model = _two_layer("detikzify-ds-7b")
    try:
        cfg = model.config.oracle_dict()
        w = weights_from_device(model, cfg, skip_prefix="vision_model.")
        ids = _text_prompt(cfg, 300, 5)
        out = model.score(ids, None, first=1)
        pos = [1, 40, 90, 129, 170, 220, 260, 299]
        per = torch.stack([torch.log_softmax(model.prefill(ids[:t], None, return_logits=True).double(), dim=-1)[ids[t]] for t in pos])
        lp16, _ = _oracle_logprobs(DetikzifyOracle(cfg, w, precision="bf16"), ids, None, 1)
        lp32, _ = _oracle_logprobs(DetikzifyOracle(cfg, w, precision="fp32"), ids, None, 1)
        sel = torch.tensor(pos) - 1
        _envelope("score at 8 positions", out.logprobs[sel], lp16[sel], lp32[sel])
        _envelope("prefill per position at 8 positions", per, lp16[sel], lp32[sel])
        print(f"score vs one prefill per position: largest |difference| {float((out.logprobs[sel].double() - per).abs().max()):.3e}")
    finally:
        del model
        gc.collect()


# ------------------------------------------------------------------------------------------ adapter
def test_text_conditioned_score():
    from detikzify_amd.model import load
    from tests.adapter_oracle import AdapterOracle
    model, proc = load("detikzify-tiny-v2", synthetic=4321, adapter=True, cross_attn_every_n_layers=2)
    w = {n: model.read_tensor(n).float().reshape(s) for n, s, _, _ in tensor_specs(TINY_V2_CFG)}
    for n in model.tensor_names():
        if n.startswith(("adapter.", "embedding_model.")):
            w[n] = model.read_tensor(n).float()
    main = {n: v for n, v in w.items() if not n.startswith(("adapter.", "embedding_model."))}
    acfg = model.adapter_config.oracle_dict()
    text = torch.randint(0, 300, (40,), generator=torch.Generator().manual_seed(3), dtype=torch.int64)
    enc = proc(images=sketch_image(1, 84), return_tensors="pt")
    prog = torch.randint(3, TINY_V2_CFG["vocab"] - 1, (24,), generator=torch.Generator().manual_seed(4))
    prog = prog[prog != TINY_V2.image_token_id]
    ids, px = torch.cat([enc.input_ids[0], prog]), enc.pixel_values
    first = model.default_first(ids)
    for tag, pixels in (("text + image", px), ("text only", None)):
        f16 = AdapterOracle(TINY_V2_CFG, acfg, w, "bf16").features(None if pixels is None else pixels[0], text)
        f32 = AdapterOracle(TINY_V2_CFG, acfg, w, "fp32").features(None if pixels is None else pixels[0], text)
        lp16, _ = _oracle_logprobs(DetikzifyOracle(TINY_V2_CFG, main, precision="bf16"), ids, px[0], first, vit_feats=f16)
        lp32, _ = _oracle_logprobs(DetikzifyOracle(TINY_V2_CFG, main, precision="fp32"), ids, px[0], first, vit_feats=f32)
        out = model.score(ids, pixels, adapter_input_ids=text)
        _envelope(f"adapter, {tag}", out.logprobs, lp16, lp32)
    plain = model.score(ids, px)
    assert not torch.equal(plain.logprobs, out.logprobs)
    # the processor's mask goes with the text, as in generate(): all ones = no mask; a padded text is refused, not scored as another prompt
    masked = model.score(ids, None, adapter_input_ids=text[None], adapter_attention_mask=torch.ones(1, 40, dtype=torch.int64))
    assert torch.equal(masked.logprobs, out.logprobs)
    with pytest.raises(NotImplementedError):
        model.score(ids, None, adapter_input_ids=text[None], adapter_attention_mask=torch.tensor([[1] * 39 + [0]]))


# ------------------------------------------------------------------------------------------ errors
def test_score_errors_reach_python_and_leave_the_context_usable(tiny):
    from detikzify_amd._lib import DtkError
    model, proc = tiny
    V, Tmax = TINY_CFG["vocab"], TINY_CFG["max_positions"]
    ids = torch.tensor([5, 6, 7, 8, 9, 10], dtype=torch.int64)
    good = model.score(ids, None, first=1)
    for bad_ids, first, msg in ((ids[:1], 1, "T >= 2"), (ids, 0, "first = 0"), (ids, 6, "first = 6"),
                                (torch.tensor([5, 6, V], dtype=torch.int64), 1, "target id"),
                                (torch.full((Tmax + 1,), 7, dtype=torch.int64), 1, "max_positions")):
        with pytest.raises(DtkError, match=msg):
            model.score(bad_ids, None, first=first)
        again = model.score(ids, None, first=1)
        assert torch.equal(again.logprobs, good.logprobs)


# ------------------------------------------------------------------------------------------ pipeline
def test_pipeline_score_sums_model_score_and_recovers_greedy_tokens(tiny):
    from detikzify_amd.infer import DetikzifyPipeline
    model, proc = tiny
    w = weights_from_device(model, TINY_CFG)
    pipe = DetikzifyPipeline(model, proc, metric="fast", compile_timeout=None)
    image = sketch_image(5, 96)
    code = "\\draw (0,0) -- (1,1);\n\\node at (2,2) {x};\n"
    total, per_token = pipe.score(image, code=code)
    tok = proc.tokenizer
    enc = proc(images=pipe.load(image), text=None, return_tensors="pt")
    ids = torch.cat([enc.input_ids[0], torch.tensor(tok.encode(code, add_special_tokens=False) + [tok.eos_token_id], dtype=torch.int64)])
    direct = model.score(ids, enc.pixel_values, first=enc.input_ids[0].numel())
    assert len(per_token) == direct.logprobs.numel() and per_token == [float(v) for v in direct.logprobs]
    assert total == float(direct.logprobs.sum(dtype=torch.float64))
    # the program greedy decoding just produced: argmax == tokens outside the fp32 oracle's near-ties.  (model.generate(do_sample=False)
    # with the prompt pipe.sample() builds, not pipe.sample() itself: sample() draws with temperature 0.8 by default, stops at EOS and
    # returns a document whose text would have to be tokenised again; the 16 greedy ids are the same kernels' output, kept as ids)
    out = model.generate(input_ids=enc.input_ids, pixel_values=enc.pixel_values, do_sample=False, max_new_tokens=16, eos_token_id=-1)
    full = out[0]
    n0 = enc.input_ids[0].numel()
    sc = model.score(full, enc.pixel_values, first=n0)
    _, rows32 = _oracle_logprobs(DetikzifyOracle(TINY_CFG, w, precision="fp32"), full, enc.pixel_values[0], n0)
    near = [top2_gap_ulps(r, [], [], False) <= 2.0 for r in rows32]
    print(f"pipeline: {sum(near)} of {len(near)} fp32-oracle rows are near-ties")
    assert 4 * sum(near) <= len(near)
    for k, (a, t) in enumerate(zip(sc.argmax.tolist(), full[n0:].tolist())):
        if not near[k]:
            assert a == t, (k, a, t)


# ------------------------------------------------------------------------------------------ timing relation
def test_score_is_not_per_row_work():
    """dtk_score of image prefix + 512 tokens < (512 x one single-sequence decode step) / 4 on ds-7b: catches a path that falls back
    to per-row work, nothing finer (tools/bench_score.py measures)."""
    from detikzify_amd.model import load
    model, proc = load("detikzify-ds-7b", synthetic=1234, max_positions=1024)
    try:
        enc = proc(images=sketch_image(0, 224), return_tensors="pt")
        g = torch.Generator().manual_seed(1)
        ids = torch.cat([enc.input_ids[0], torch.randint(3, 31000, (512,), generator=g)])
        px = enc.pixel_values
        model.score(ids, px)                       # warm-up: workspace, code objects
        t_score = []
        for _ in range(3):
            t0 = time.perf_counter(); model.score(ids, px); t_score.append(time.perf_counter() - t0)
        model.set_sampling(do_sample=False)
        model.prefill(ids[:-64], px)
        for _ in range(8):
            model.decode_launch(); model.decode_wait()
        t0 = time.perf_counter()
        for _ in range(32):
            model.decode_launch(); model.decode_wait()
        step = (time.perf_counter() - t0) / 32
        b, c = sorted(t_score)[1], 512 * step
        print(f"ds-7b: score of {ids.numel()} tokens {b * 1e3:.1f} ms (host wall time), 512 decode steps {c * 1e3:.1f} ms, ratio {c / b:.1f}")
        assert b < c / 4
    finally:
        del model
        gc.collect()
