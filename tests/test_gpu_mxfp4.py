"""
weight_format="mxfp4" on the GPU (-m gpu): the MXFP4 decode GEMV op by op (dtk_op_gemv_q4 = the loader's quantiser + the shipped
k_gemv instantiation) against tests/mxfp4_ref.py in float64, the loader's quantiser through load_tensor / read_tensor, and a toy model
end to end against the CPU oracle on the effective weights — with the bounds of test_op_gemv and of
test_fp8_weights_parity_and_quantisation_error (tests/test_gpu_parity.py), which this mirrors for the new format.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sampling
from oracle.llama import rmsnorm
from oracle.model import DetikzifyOracle
from oracle.ops import bits_to_f32, f32_to_bits, rb
from oracle.synth import tensor_specs
from tests import mxfp4_ref as ref
from tests.helpers import TINY, rel_l2, sketch_image

SHAPES = [(1, 32), (37, 48), (256, 688), (100, 2048), (37, 4096), (512, 5504)]
E2M1 = np.concatenate([ref.GRID, -ref.GRID])         # value of code c (c & 8 = sign)


@pytest.fixture(scope="module")
def ctx_model():
    """any context serves the op (it brings its own weights)"""
    from detikzify_amd.model import load
    return load("detikzify-tiny", synthetic=1234)[0]


def _bits(a):
    return f32_to_bits(torch.as_tensor(np.asarray(a, dtype=np.float32)))


def gemv_q4(model, W, x, norm_w=None, mode=0, eps=1e-6):
    """(y [N], W_eff [N][K]) as float32 numpy; W / x / norm_w must be bf16-representable"""
    W = np.asarray(W, dtype=np.float32)
    N, K = W.shape
    Wb, xb = _bits(W), _bits(x)
    nb = _bits(norm_w) if norm_w is not None else np.zeros(K, dtype=np.uint16)
    assert np.array_equal(bits_to_f32(Wb).numpy(), W) and np.array_equal(bits_to_f32(xb).numpy(), np.asarray(x, dtype=np.float32))
    y, weff = np.empty(N, dtype=np.uint16), np.empty((N, K), dtype=np.uint16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    model._check(model.lib.dtk_op_gemv_q4(model._ctx, p(Wb), p(xb), p(nb), N, K, mode, eps, p(y), p(weff)), "dtk_op_gemv_q4")
    return bits_to_f32(y).numpy(), bits_to_f32(weff).numpy()


# ------------------------------------------------------------------------------------------ 1. decode table
def _table(K, shift):
    """16 rows x K: code (n + k + block + shift) % 16 at position k of row n, block exponent (-20, 0, +8)[(n + block + shift) % 3].  Over
    the 16 rows every position sees all 16 codes and all three exponents, but code and exponent both follow n, so a position sees 16 (per
    shift; 18 over the three shifts at K = 32) of the 48 (code, exponent) pairs, not all of them.  Every block holds +-6 (every code
    twice), so its scale is exactly its exponent."""
    n, k = np.arange(16)[:, None], np.arange(K)[None, :]
    code = (n + k + k // 32 + shift) % 16
    e = np.array([-20, 0, 8])[(n + k // 32 + shift) % 3]
    return E2M1[code] * np.exp2(e.astype(np.float64)), e


@pytest.mark.parametrize("K", [32, 2080])
def test_decode_table_one_hot(ctx_model, K):
    """y[n] = W_eff[n][k] exactly for a one-hot x at every k: pins the nibble order, the scale byte and the lane / chunk mapping
    (K = 2080 = 65 blocks: a wave-load covers 2048 weights, so the second round has one live lane)"""
    for shift in ((0, 1, 2) if K == 32 else (0,)):
        W, e = _table(K, shift)
        codes, scales, W_eff = ref.quantise(W)
        assert np.array_equal(W_eff, W) and np.array_equal(scales, (e[:, ::32] + 127).astype(np.uint8))   # the table is its own quantisation
        for k in range(K):
            x = np.zeros(K, dtype=np.float32)
            x[k] = 1.0
            y, weff = gemv_q4(ctx_model, W, x)
            if k == 0:
                assert np.array_equal(weff, W.astype(np.float32)), "quantiser: de-quantised table"
            assert np.array_equal(y, W[:, k].astype(np.float32)), (K, shift, k, y, W[:, k])


# ------------------------------------------------------------------------------------------ 2. grid operands (exact sums)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("N,K", SHAPES)
def test_grid_operands_bit_exact(ctx_model, N, K, mode):
    """W = E2M1 values x 2^e with e in {-1, 0, 1} per block, x multiples of 1/8 with |x| <= 2: every product is a multiple of
    2^-2 * 2^-3 = 2^-5 and |sum| <= K * 12 * 2 < 2^18 at K <= 5504, so every partial sum in any order fits the 24 bits of fp32 — the kernel
    must return the bf16 rounding of the exact float64 sum.  Mode 1 keeps the grid: |x| = 1 everywhere, so mean(x^2) = 1, x * rsqrt(1 + eps)
    rounds to +-1 in bf16, and the normalised input is +-norm_w with norm_w on the 1/8 grid."""
    rng = np.random.default_rng(1000 * mode + N + K)
    KC = (K + 31) // 32
    e_blk = rng.integers(-1, 2, size=(N, KC))
    W = rng.choice(E2M1, size=(N, KC * 32)) * np.repeat(np.exp2(e_blk.astype(np.float64)), 32, axis=1)
    W[:, ::32] = 6.0 * np.exp2(e_blk.astype(np.float64)) * rng.choice([-1.0, 1.0], size=(N, KC))     # pins the block scale: W is its own quantisation
    W = W[:, :K]
    grid = rng.integers(-16, 17, size=K) / 8.0
    if mode == 0:
        x, nw, xin = grid, None, grid
    else:
        x = rng.choice([-1.0, 1.0], size=K)
        nw = grid
        xin = x * nw
        assert np.array_equal(rmsnorm(torch.tensor(x, dtype=torch.float32), torch.tensor(nw, dtype=torch.float32), 1e-6).numpy(), xin.astype(np.float32))
    assert np.array_equal(ref.quantise(W)[2], W)
    y, weff = gemv_q4(ctx_model, W, x, nw, mode)
    assert np.array_equal(weff, W.astype(np.float32))
    exact = ref.gemv_ref(W, xin)
    assert float(np.abs(exact).max()) < 2.0 ** 18
    want = rb(torch.tensor(exact, dtype=torch.float64).float()).numpy()       # exact in fp32, then the one bf16 rounding of the output
    bad = np.flatnonzero(y != want)
    assert bad.size == 0, (N, K, mode, bad[:8], y[bad[:8]], want[bad[:8]])


# ------------------------------------------------------------------------------------------ 3. random operands
def _ulp_report(got, ref_f32):
    """tests/test_gpu_parity.py::ulp_report: fraction of elements that differ, max difference in bf16 ulps of the reference, rel-L2"""
    got = torch.as_tensor(got, dtype=torch.float32).reshape(-1)
    r = rb(torch.as_tensor(ref_f32, dtype=torch.float32)).reshape(-1)
    diff = (got - r).abs()
    ulp = torch.clamp(r.abs(), min=1e-2 * float(r.abs().max()) + 1e-30) * 2.0 ** -7
    return float((diff > 0).float().mean()), float((diff / ulp).max()), rel_l2(got, r)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("N,K", SHAPES)
def test_random_operands(ctx_model, N, K, mode):
    """test_op_gemv's bars against the float64 product of the de-quantised weights the op returns (themselves checked against the
    reference quantiser): rel-L2 < 1e-3, <= 2.01 bf16 ulps, < 5 % of the elements differing"""
    g = torch.Generator().manual_seed(N + K + 7 * mode)
    W = rb(torch.randn(N, K, generator=g) * 0.05); x = rb(torch.randn(K, generator=g))
    nw = rb(1 + 0.1 * torch.randn(K, generator=g))
    xin = rmsnorm(x, nw, 1e-6) if mode == 1 else x
    y, weff = gemv_q4(ctx_model, W.numpy(), x.numpy(), nw.numpy(), mode)
    assert np.array_equal(weff, ref.quantise(W.numpy())[2].astype(np.float32)), "de-quantised weights != reference quantiser"
    want = ref.gemv_ref(weff, xin.numpy())
    frac, ulps, rl2 = _ulp_report(y, want)
    print(f"gemv_q4 {N}x{K} mode={mode}: differing {frac:.4f} max_ulp {ulps:.2f} rel_l2 {rl2:.2e}")
    assert rl2 < 1e-3 and ulps <= 2.01 and frac < 0.05


# ------------------------------------------------------------------------------------------ 4. the loader's quantiser
@pytest.fixture(scope="module")
def tiny_pair():
    from detikzify_amd.model import load
    m4, proc = load("detikzify-tiny", synthetic=1234, weight_format="mxfp4")
    m16, _ = load("detikzify-tiny", synthetic=1234)
    return m4, m16, proc


def _crafted(N, K, seed):
    """random bf16 rows with the special cases planted: the E2M1 ties at a block whose amax is 6 * 2^e, amax with mantissa 1.5 and the
    next bf16 above it, an all-zero block, a zero row"""
    g = torch.Generator().manual_seed(seed)
    W = rb(torch.randn(N, K, generator=g) * 0.03).numpy().astype(np.float64)
    ties = np.array([6.0, 2.5, 3.5, 5.0, 0.25, 0.75, 1.25, 1.75, -2.5, -3.5, -5.0, -0.25, -0.75, 3.0, -6.0, 0.5])
    W[0, :32] = 0.0; W[0, :16] = ties * 2.0 ** -9
    W[1, 32:64] = 0.0; W[1, 32:48] = ties * 2.0 ** 3
    W[2, :32] = np.clip(W[2, :32], -1.0, 1.0) * 2.0 ** -6; W[2, 5] = 1.5 * 2.0 ** -6
    W[3, :32] = np.clip(W[3, :32], -1.0, 1.0) * 2.0 ** -6; W[3, 9] = -(1.5 + 2.0 ** -7) * 2.0 ** -6
    W[4, 64:96] = 0.0
    W[5, :] = 0.0
    W[6, K - (K % 32 or 32):] *= 2.0 ** -5            # the last (ragged, where K % 32) block on a scale of its own
    W[7, K - (K % 32 or 32):] = 0.0; W[7, K - 1] = 2.5 * 2.0 ** -4; W[7, K - 2] = -6.0 * 2.0 ** -4
    return W


def test_loader_quantiser_matches_reference(tiny_pair):
    m4, m16, _ = tiny_pair
    d, ff = TINY.hidden, TINY.ffn
    assert ff % 32 == 16
    for name, (N, K) in {"model.layers.1.mlp.down_proj.weight": (d, ff), "model.layers.0.mlp.gate_proj.weight": (ff, d),
                         "model.layers.1.self_attn.o_proj.weight": (d, d), "model.layers.0.self_attn.k_proj.weight": (d, d)}.items():
        before = m4.read_tensor(name).float().numpy().reshape(N, K)                       # the synthetic fill, quantised at first use
        assert np.array_equal(before, ref.quantise(m16.read_tensor(name).float().numpy().reshape(N, K))[2].astype(np.float32)), name
        W = _crafted(N, K, N + K)
        m4.load_tensor(name, torch.tensor(W, dtype=torch.float32))                          # re-quantised lazily, as in fp8 mode
        got = m4.read_tensor(name).float().numpy().reshape(N, K)
        want = ref.quantise(W)[2]
        bad = np.argwhere(got != want.astype(np.float32))
        assert bad.size == 0, (name, bad[:6], [(got[tuple(b)], want[tuple(b)], W[tuple(b)]) for b in bad[:6]])
        for c in range((K + 31) // 32):
            blk = slice(c * 32, min(K, (c + 1) * 32))
            assert np.all(np.abs(got[:, blk] - W[:, blk]) <= 0.25 * np.abs(W[:, blk]).max(axis=1, keepdims=True)), (name, c)
        m4.load_tensor(name, m16.read_tensor(name).reshape(N, K))                           # restore the synthetic weights
        assert np.array_equal(m4.read_tensor(name).float().numpy().reshape(N, K), before)
    for name in ("model.norm.weight", "model.embed_tokens.weight", "model.layers.0.input_layernorm.weight", "model.mm_projector.bias"):
        assert torch.equal(m4.read_tensor(name), m16.read_tensor(name)), name                # not quantised
    # lm_head takes the fp8 path: e4m3 values times a per-row power of two (the fp8 test's statement)
    w8 = m4.read_tensor("lm_head.weight").float().view(TINY.vocab, d)
    w16 = m16.read_tensor("lm_head.weight").float().view(TINY.vocab, d)
    amax = w16.abs().amax(dim=1, keepdim=True)
    scale = torch.exp2(torch.ceil(torch.log2(amax / 448.0)))
    q = w8 / scale
    assert torch.equal(q, q.to(torch.float8_e4m3fn).float())
    assert float(((w8 - w16).abs() / (amax + 1e-30)).max()) <= 2.0 ** -4 + 1e-6


# ------------------------------------------------------------------------------------------ 5. model level
def _device_weights(model, cfg):
    out = {}
    for name, shape, _, _ in tensor_specs(cfg):
        if name.startswith("rope."):
            shape = (cfg["max_positions"], cfg["head_dim"] // 2)
        out[name] = model.read_tensor(name).float().reshape(shape)
    return out


def _greedy(model, ids, px, n, graph=1):
    model.set_graph_mode(graph)
    out = model.generate(input_ids=ids[None], pixel_values=px, do_sample=False, max_new_tokens=n,
                         bad_words_ids=[[model.config.image_token_id]], begin_suppress_tokens=[2], eos_token_id=-1)
    model.set_graph_mode(1)
    return out[0, ids.numel():].tolist()


@pytest.mark.parametrize("name", ["detikzify-tiny", "detikzify-tiny-tl"])
def test_mxfp4_model_matches_oracle_on_effective_weights(name):
    """Prefill and 32 greedy decode steps against DetikzifyOracle built from the weights read back from the device (parity is defined
    against the effective weights, as for fp8), with that test's bounds; the quantisation shift against the bf16 model is reported."""
    from detikzify_amd.model import load
    m4, proc = load(name, synthetic=1234, weight_format="mxfp4")
    m16, _ = load(name, synthetic=1234)
    cfg = m4.config.oracle_dict()
    oracle = DetikzifyOracle(cfg, _device_weights(m4, cfg), precision="bf16")
    enc = proc(images=sketch_image(2, 96), return_tensors="pt")
    ids, px = enc.input_ids[0], enc.pixel_values
    lo = m4.prefill(ids, px, return_logits=True)
    r = rel_l2(lo, oracle.prefill(ids, px[0]))
    shift = rel_l2(lo, m16.prefill(ids, px, return_logits=True))
    toks = _greedy(m4, ids, px, 32)
    logits, flips, worst = oracle.prefill(ids, px[0]), 0, 0.0
    m4.set_sampling(do_sample=False, bad_ids=[1], begin_suppress_ids=[2])
    m4.prefill(ids, px)
    for i, t in enumerate(toks):
        rt = sampling.greedy(logits, [1], [2], i == 0)
        if rt != t:
            top2 = torch.topk(sampling.mask_scores(logits, [1], [2], i == 0), 2)[0]
            assert float(top2[0] - top2[1]) <= 2 * float(top2[0].abs()) * 2.0 ** -7 + 1e-6, (i, t, rt)
            flips += 1
        m4.decode_launch()
        assert m4.decode_wait() == t
        logits = oracle.step(t)
        worst = max(worst, rel_l2(m4.get_logits(), logits))
    st4, st16 = m4.stats(), m16.stats()
    ratio = st4["weight_bytes_per_token"] / st16["weight_bytes_per_token"]
    print(f"mxfp4 {name}: prefill logits vs oracle(effective weights) {r:.2e}; decode worst {worst:.2e}; {flips} near-tie flips; "
          f"quantisation shift vs bf16 weights {shift:.2e}; weight bytes per token {ratio:.3f} of bf16")
    assert r < 1e-2 and worst < 1e-2 and flips <= 3
    assert np.isfinite(shift) and shift > 0
    assert ratio < 0.31          # layers 4.25 / 16 = 0.266, lm_head 0.5 + scales: detikzify-tiny 0.285 with the padded down_proj
    # graph replay == plain launches; a sampled run with a fixed seed repeats its tokens
    assert _greedy(m4, ids, px, 32, graph=0) == toks
    kw = dict(do_sample=True, temperature=0.8, top_p=0.95, top_k=0, seed=99, max_new_tokens=24,
              bad_words_ids=[[1]], begin_suppress_tokens=[2], eos_token_id=-1)
    a = m4.generate(input_ids=ids[None], pixel_values=px, **kw)[0, ids.numel():].tolist()
    assert a == m4.generate(input_ids=ids[None], pixel_values=px, **kw)[0, ids.numel():].tolist() and len(set(a)) > 4


# ------------------------------------------------------------------------------------------ 6. refusal
def test_dtk_create_refuses_mxfp4_with_batch_slots():
    from detikzify_amd import _lib
    from detikzify_amd.model.config import preset
    from detikzify_amd.model.modeling import DetikzifyForCausalLM
    cfg = preset("detikzify-tiny")
    cfg.batch_slots, cfg.weight_format = 2, "mxfp4"
    with pytest.raises(_lib.DtkError, match="MXFP4 weights have no batched-slot or multi-vector kernels yet"):
        DetikzifyForCausalLM(cfg, 0)


# ------------------------------------------------------------------------------------------ 7. the per-role timing aid
@pytest.mark.parametrize("fmt", ["bf16", "fp8", "mxfp4"])
def test_bench_gemv_streams_the_contexts_format(fmt):
    """dtk_bench_gemv with 0xff | 0x800 (what tools/bench_mxfp4.py calls): every role of a toy context in each weight format runs its
    shipped kernel on the format's own arrays and reports a positive time; the context decodes as before afterwards."""
    from detikzify_amd.model import load
    m, proc = load("detikzify-tiny", synthetic=1234, weight_format=fmt)
    enc = proc(images=sketch_image(2, 96), return_tensors="pt")
    ids, px = enc.input_ids[0], enc.pixel_values
    toks = _greedy(m, ids, px, 8)
    for role in range(5):
        us = C.c_float(0.0)
        m._check(m.lib.dtk_bench_gemv(m._ctx, role, 0xFF | 0x800, 2, C.byref(us)), "dtk_bench_gemv")
        assert np.isfinite(us.value) and us.value > 0, (fmt, role, us.value)
    us = C.c_float(0.0)
    assert m.lib.dtk_bench_gemv(m._ctx, 2, 0 | 0x800, 2, C.byref(us)) != 0        # the format bit goes with the shipped kernel (0xff) only
    assert _greedy(m, ids, px, 8) == toks
