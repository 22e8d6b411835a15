"""The 13-bit planes of bf16 weight rows (csrc/w13.h) on the device: the kernels rebuild the rows' own bits and fold them in the bf16
kernel's order, so the bar everywhere in this file is BIT EQUALITY with the bf16 format, never a tolerance.

Op level (dtk_op_gemv_role, variant 0x1000 + shape: the packer + one role on host operands): every (prologue, epilogue) pair of a
layer plus LOGITS and the STORE pairs, every 13-bit shape, against the bf16 kernel with the same fold order (any shape without split-K;
the split-K twin for a split-K shape); every result buffer starts as NaN poison, so a cell the role does not own must still hold it
(compared as bytes); a matrix with an unpackable row must run the bf16 kernel.  Model level: 32 greedy steps of the toy models with
option w13 = 1 against 0; the packer's counters; the packer on the benchmark's synthetic ds-7b."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import gemv_cases as gc
from tests.test_gpu_gemv import _call, _operands, _run, _same

pytestmark = pytest.mark.gpu

W13 = 0x1000
K_LIST = (72, 512, 520, 1032, 1544)        # one ragged unit; half a unit; + one chunk; one unit + a chunk; a sign block and a ragged unit
N_LIST = (1, 37, 130)
FF_LIST = (8, 24, 88)
HEADS = ((2, 2), (4, 1))
K_NORM = (4096, 4104)                      # RMSNorm roles: x spans every wave of a 4- and of an 8-wave block (both paths of the prologue)
# 13-bit shapes of a role (kernels_decode.hip: launch_gemv_w13_variant) -> a bf16 variant with the same fold order: the same split-K
# grouping, and for PRO_RMSNORM the same number of waves (the sum of squares is folded per thread, wave and block: K_NORM shows it)
SHAPES = {
    (gc.RMSNORM, gc.QKV): {0: 0, 1: 0, 2: 10, 3: 10, 4: 0, 5: 0},
    (gc.RMSNORM, gc.SWIGLU): {0: 0, 1: 0, 2: 10, 3: 10, 4: 0, 5: 0},
    (gc.COPY, gc.RESID): {0: -1, 1: -1, 2: -1, 3: 13, 4: 14, 5: -1, 6: -1},      # 3, 4: split-K 2 over groups of 4 k-iterations
    (gc.ATTN, gc.RESID): {0: 8, 1: 1, 2: 1},                       # 0: split-K 2 (the d > 2048 default)
    (gc.RMSNORM, gc.LOGITS): {0: 3, 1: 3, 2: 1, 3: 1, 4: 1},
    (gc.RMSNORM, gc.STORE): {0: -1},
    (gc.COPY, gc.STORE): {0: -1},
}


@pytest.fixture(scope="module")
def tiny():
    from detikzify_amd.model import load
    return load("detikzify-tiny", synthetic=1234)[0]


def cases(pro, epi):
    if epi == gc.QKV:          # K = d = H * hd
        return [gc.Case(pro, epi, "bf16", K=H * hd, H=H, KVH=KVH, hd=hd, pos=pos) for hd in (128, 64) for H, KVH in HEADS for pos in (0, gc.T_MAX - 1)]
    if epi == gc.SWIGLU:
        return [gc.Case(pro, epi, "bf16", K=K, ff=ff) for K in K_LIST for ff in FF_LIST] + [gc.Case(pro, epi, "bf16", K=K, ff=24) for K in K_NORM]
    if pro == gc.ATTN:         # K = H * hd
        return [gc.Case(pro, epi, "bf16", N=N, H=H, hd=hd, S=S) for hd in (128, 64) for H, _ in HEADS for S in (1, 4, 5) for N in (N_LIST if S == 4 else N_LIST[S % 3:][:1])]
    return [gc.Case(pro, epi, "bf16", K=K, N=N) for K in K_LIST for N in N_LIST] + [gc.Case(pro, epi, "bf16", K=K, N=37) for K in K_NORM if pro == gc.RMSNORM]


@pytest.mark.parametrize("role", sorted(SHAPES), ids=lambda r: f"{gc.PRO_NAME[r[0]]}-{gc.EPI_NAME[r[1]]}")
def test_op_bit_equal_to_bf16(tiny, role):
    pro, epi = role
    n = 0
    for case in cases(pro, epi):
        ref = {}
        for shape, twin in SHAPES[role].items():
            if twin not in ref:
                ref[twin] = _run(tiny, case, twin)
            got = _run(tiny, case, W13 + shape)
            assert tiny.lib.dtk_w13_op_bad_rows(tiny._ctx) == 0, case.name           # the planes were streamed, not the bf16 rows
            assert _same(got, ref[twin]), f"{case.name}: 13-bit shape {shape} differs from bf16 variant {twin}"
            n += 1
        got = _run(tiny, case, W13 + 0xFF)                                             # the shape launch_gemv picks
        assert _same(got, ref.setdefault(-1, _run(tiny, case, -1))), f"{case.name}: the step's 13-bit shape differs from the step's bf16 kernel"
    print(f"{gc.PRO_NAME[pro]}-{gc.EPI_NAME[epi]}: {n} (case, shape) pairs bit-equal")


def test_poison_survives_in_cells_the_role_does_not_own(tiny):
    """QKV writes row `pos` of the caches only; every other row still holds its NaN poison after the 13-bit kernel, as after the bf16 one"""
    case = gc.Case(gc.RMSNORM, gc.QKV, "bf16", K=256, H=2, KVH=2, hd=128, pos=3)
    before, got = case.initial(), _run(tiny, case, W13)
    for n in ("k", "v"):
        rows_b, rows_g = before[n].reshape(2, gc.T_MAX, 128), got[n].reshape(2, gc.T_MAX, 128)
        keep = np.arange(gc.T_MAX) != 3
        assert np.array_equal(rows_b[:, keep].view(np.uint8), rows_g[:, keep].view(np.uint8))
        assert not np.array_equal(rows_b[:, 3].view(np.uint8), rows_g[:, 3].view(np.uint8))


@pytest.mark.parametrize("role", [(gc.RMSNORM, gc.SWIGLU), (gc.COPY, gc.RESID), (gc.RMSNORM, gc.LOGITS)], ids=lambda r: gc.EPI_NAME[r[1]])
def test_unpackable_row_takes_the_bf16_kernel(tiny, role):
    pro, epi = role
    case = gc.Case(pro, epi, "bf16", K=520, ff=24) if epi == gc.SWIGLU else gc.Case(pro, epi, "bf16", K=520, N=37)
    o = _operands(case)
    W = o["W"].copy()
    row = W[5]
    hb = int(((row >> 8) & 0x7F).max())
    assert hb > 16
    row[K_AT] = ((hb - 15) << 8) | 0x33                  # one weight 30 binades below the row's largest: outside the window
    o["W"] = W
    try:
        want = _run(tiny, case, -1)                      # the bf16 kernel on the changed matrix
        for v in (W13, W13 + 0xFF):
            got = _run(tiny, case, v)
            assert tiny.lib.dtk_w13_op_bad_rows(tiny._ctx) == 1
            assert _same(got, want)
    finally:
        del case.dev


K_AT = 257


def test_refusals(tiny):
    case = gc.Case(gc.COPY, gc.RESID, "bf16", K=72, N=37)
    for v in (W13 + 7, W13 + 0xFE, W13 + 0x100):
        rc, _ = _call(tiny, case, v)
        assert rc == -1, v


@pytest.mark.parametrize("name", ["detikzify-tiny", "detikzify-tiny-tl"])
def test_decode_logits_and_tokens_identical(name):
    from detikzify_amd.model import load
    from tests.helpers import sketch_image
    model, proc = load(name, synthetic=1234)
    enc = proc(images=sketch_image(0, 96), return_tensors="pt")
    ids, px = enc.input_ids[0], enc.pixel_values
    L = model.config.layers
    runs = {}
    for w13 in (0, 1):
        model.set_option("w13", w13)
        model.set_sampling(do_sample=False, bad_ids=[1], begin_suppress_ids=[2])
        model.prefill(ids, px)
        logits, toks = [model.get_logits().clone()], []
        for _ in range(32):
            model.decode_launch()
            toks.append(model.decode_wait())
            logits.append(model.get_logits().clone())
        runs[w13] = (toks, logits, model.stats())
    assert runs[0][0] == runs[1][0]
    for i, (a, b) in enumerate(zip(runs[0][1], runs[1][1])):
        assert np.array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32)), f"logits of step {i} differ"
    c0, c1 = runs[0][2]["w13_counts"], runs[1][2]["w13_counts"]
    assert c0 == 0
    packed, unpacked, bad_rows = c1 & 1023, (c1 >> 10) & 1023, c1 >> 20
    # q/k/v, gate/up and lm_head.  o_proj keeps its bf16 rows at any size (measured slower on planes), and at d <= 2048 down's bf16 default is
    # a split-K shape over groups of 6 k-iterations, which has no 13-bit twin
    assert (packed, unpacked, bad_rows) == (2 * L + 1, 0, 0)
    # the bytes the step streams: planes (whole units of 1024 weights + the sign blocks: LARGER than a toy row) + the row byte for q/k/v,
    # gate/up and lm_head, bf16 rows for o_proj and down, bf16 norm vectors
    cfg = model.config
    d, ff, V, kvd = cfg.hidden, cfg.ffn, cfg.vocab, cfg.num_kv_heads * cfg.head_dim
    units = -(-d // 1024)
    row = units * 1536 + -(-units // 2) * 256 + 1
    want = L * ((d + 2 * kvd) * row + 2 * ff * row + 2 * d * d + 2 * d * ff + 4 * d) + 2 * d + V * row
    assert runs[1][2]["weight_bytes_per_token"] == want
    assert runs[0][2]["weight_bytes_per_token"] == 2 * (L * (2 * d * d + 2 * kvd * d + 3 * d * ff + 2 * d) + d + V * d)


def test_packer_takes_every_matrix_of_the_benchmarks_model():
    """the synthetic ds-7b of bench.py: no matrix has an unpackable row (asserted, not assumed: the generator draws on a 2^-23 grid)"""
    from detikzify_amd.model import load
    model, _ = load("detikzify-ds-7b", synthetic=1234)
    model.set_option("w13", 1)
    us = C.c_float(0.0)
    model._check(model.lib.dtk_bench_gemv(model._ctx, 2, 0xFF, 1, C.byref(us)), "dtk_bench_gemv")     # what the step streams: packs; no decode needed
    c = model.stats()["w13_counts"]
    L = model.config.layers
    assert (c & 1023, (c >> 10) & 1023, c >> 20) == (3 * L + 1, 0, 0)          # q/k/v, gate/up, down of every layer + lm_head; unpacked 0
    st = model.stats()
    assert st["weight_bytes_per_token"] < 0.84 * 13_216_784_384                  # 13 / 16 of every packed role (K = 11008: 0.837), o_proj bf16: 0.833
