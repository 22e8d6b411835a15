"""The 13-bit kernels' two freedoms on the device, bar BIT EQUALITY with the bf16 kernel everywhere (bytes over NaN-poisoned buffers):

(1) the shapes of 8 and 16 waves that fold the RMSNorm sum of squares as a 4-wave block does (k_gemv's FW) against the 4-wave bf16
    variant, at K = 4096 / 4104 on the seeds of tests/w13_fold.NORM_CASES, where tests/test_w13_fold_host.py shows the block's own
    fold to give another `inv`;
(2) rows with and without a zero code (w13.h: W13_ZROW in the device's row byte): a wave takes the short decode only when none of
    its rows has the bit - no row flagged, every row flagged, exactly one row of a wave's group, and a persistent wave whose second
    row group is flagged differently from its first;
(3) the toy models with zeros planted in a q/k/v and a gate row, 32 greedy steps, w13 = 1 against 0; the packer on the benchmark's model."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import gemv_cases as gc
from tests import w13_fold as wf
from tests.test_gpu_gemv import _operands, _p, _run, _same

pytestmark = pytest.mark.gpu

W13 = 0x1000
ZROW = 0x80
ROLE_ID = lambda r: f"{gc.PRO_NAME[r[0]]}-{gc.EPI_NAME[r[1]]}"
ZERO_PATTERNS = (0x0000, 0x8000, 0x0001, 0x807F, 0x00C5, 0x80FF)          # +-0, two denormals, two e = 1 patterns: e >> 1 == 0, code 0


@pytest.fixture(scope="module")
def tiny():
    from detikzify_amd.model import load
    return load("detikzify-tiny", synthetic=1234)[0]


def _row_bytes(model, W):
    out = np.zeros(W.shape[0], np.uint8)
    assert model.lib.dtk_w13_row_bytes_host(_p(W), W.shape[0], W.shape[1], _p(out)) == 0
    return out


def _planes_streamed(model, name):
    assert model.lib.dtk_w13_op_bad_rows(model._ctx) == 0, name            # the planes were streamed, not the bf16 rows


# ------------------------------------------------------------------------------------------ (1) the new shapes, fold of 4 waves
def _ragged(role):
    pro, epi = role
    for K in (72, 520):
        if epi == gc.QKV:
            yield gc.Case(pro, epi, "bf16", K=K, H=2, KVH=1, hd=64, pos=gc.POS_IN)
        elif epi == gc.SWIGLU:
            yield gc.Case(pro, epi, "bf16", K=K, ff=24)
        else:
            yield gc.Case(pro, epi, "bf16", K=K, N=37)


@pytest.mark.parametrize("role", sorted(wf.NEW), ids=ROLE_ID)
def test_new_shapes_equal_the_bf16_variant_of_equal_fold(tiny, role):
    pro, epi = role
    cases = list(_ragged(role)) + [gc.Case(pro, epi, "bf16", seed=seed, **({"pos": gc.POS_IN} if epi == gc.QKV else {}), **kw)
                                   for r, kw, seed in wf.NORM_CASES if r == role]
    assert len(cases) == 4
    n = 0
    for case in cases:
        ref = {}
        for shape, twin in wf.NEW[role].items():
            if twin not in ref:
                ref[twin] = _run(tiny, case, twin)
            got = _run(tiny, case, W13 + shape)
            _planes_streamed(tiny, case.name)
            assert _same(got, ref[twin]), f"{case.name}: 13-bit shape {shape} differs from bf16 variant {twin}"
            n += 1
    print(f"{ROLE_ID(role)}: {n} (case, shape) pairs bit-equal")


# ------------------------------------------------------------------------------------------ (2) zero codes
def _zero_case(role, K):
    pro, epi = role
    if epi == gc.QKV:
        return gc.Case(pro, epi, "bf16", K=K, H=2, KVH=1, hd=64, pos=gc.POS_IN)
    if epi == gc.SWIGLU:
        return gc.Case(pro, epi, "bf16", K=K, ff=24)
    return gc.Case(pro, epi, "bf16", K=K, N=37)


def _plant(W, rows, K):
    """code-0 weights in the first, a middle and the last chunk of each row, and in the first chunk of the ragged last unit"""
    K8 = K // 8
    at = [3, (K8 // 2) * 8 + 5, K - 1, (K8 // 128) * 128 * 8 + 2]
    assert K8 % 128 != 0 and at[3] < K
    for i, r in enumerate(rows):
        for j, k in enumerate(at):
            W[r, k] = ZERO_PATTERNS[(i + j) % len(ZERO_PATTERNS)]
    return W


def _one_row_per_group(role, case):
    """rows to flag so that a wave's group (R 1 and R 2 shapes alike) holds exactly one flagged row"""
    pro, epi = role
    if epi == gc.SWIGLU:          # unit u = rows (u, ff + u); R 2 groups units (2j, 2j + 1): gate only, up only, gate only
        return [0, case.ff + 3, 6]
    if epi == gc.QKV:             # hd 64: unit u = rows (r0, r0 + 32) of a head: a q row, a RoPE partner alone, a k row, a v partner
        return [1, 32 + 4, 2 * 64 + 7, 3 * 64 + 32 + 10]
    return [0, 3, 36]             # R 2 groups rows (2j, 2j + 1): the first, the second, the lone last


@pytest.mark.parametrize("K", (520, 1544))
@pytest.mark.parametrize("role", sorted(wf.TWIN), ids=ROLE_ID)
def test_zero_code_rows(tiny, role, K):
    case = _zero_case(role, K)
    o = _operands(case)
    W0 = o["W"].copy()
    mats = {"none": W0,
            "all": _plant(W0.copy(), range(case.N), K),
            "one": _plant(W0.copy(), _one_row_per_group(role, case), K)}
    assert not (_row_bytes(tiny, mats["none"]) & ZROW).any()
    assert (_row_bytes(tiny, mats["all"]) & ZROW).all()
    flagged = np.flatnonzero(_row_bytes(tiny, mats["one"]) & ZROW).tolist()
    assert flagged == sorted(_one_row_per_group(role, case))
    n = 0
    try:
        for what, W in mats.items():
            o["W"] = W
            ref = {}
            for shape, twin in wf.TWIN[role].items():
                if twin not in ref:
                    ref[twin] = _run(tiny, case, twin)
                got = _run(tiny, case, W13 + shape)
                _planes_streamed(tiny, case.name)
                assert _same(got, ref[twin]), f"{case.name}, rows flagged: {what}: 13-bit shape {shape} differs from bf16 variant {twin}"
                n += 1
    finally:
        del case.dev
    print(f"{ROLE_ID(role)} K {K}: {n} (matrix, shape) pairs bit-equal")


def test_persistent_second_trip_with_another_flag(tiny):
    """K = 64 and more units than the grid's first round by less than a round: the waves with a second row group find it flagged when
    the first was not, and the other way round"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 0
    for role in sorted(wf.TWIN):
        pro, epi = role
        for shape, (R, U, waves, bpc, fw) in sorted(wf.TABLE13[role].items()):
            if not bpc:
                continue
            first = cus * bpc * waves * R
            if epi == gc.QKV:
                H = -(-first // 64) - 1
                case = gc.Case(pro, epi, "bf16", K=64, H=H, KVH=1, hd=128, pos=gc.POS_IN)
            elif epi == gc.SWIGLU:
                case = gc.Case(pro, epi, "bf16", K=64, ff=(first + 40 + 7) // 8 * 8)
            else:
                case = gc.Case(pro, epi, "bf16", K=64, N=first + 37)
            assert first < case.units < 2 * first, (case.name, first, case.units)
            o = _operands(case)
            W0 = o["W"].copy()
            unit_of_row = np.arange(case.N)
            if epi == gc.QKV:
                unit_of_row = (unit_of_row // 128) * 64 + unit_of_row % 64
            elif epi == gc.SWIGLU:
                unit_of_row = unit_of_row % case.ff
            try:
                for late in (True, False):
                    W = W0.copy()
                    W[(unit_of_row >= first) == late, 5] = 0x8000
                    o["W"] = W
                    want = _run(tiny, case, wf.TWIN[role][shape])
                    got = _run(tiny, case, W13 + shape)
                    _planes_streamed(tiny, case.name)
                    assert _same(got, want), f"{case.name}: 13-bit shape {shape}, rows of the {'second' if late else 'first'} round flagged"
                    n += 1
            finally:
                del case.dev
    print(f"{n} (shape, flag order) pairs bit-equal")


# ------------------------------------------------------------------------------------------ (3) models
@pytest.mark.parametrize("name", ["detikzify-tiny", "detikzify-tiny-tl"])
def test_decode_with_planted_zeros_identical(name):
    import torch
    from detikzify_amd.model import load
    from tests.helpers import sketch_image
    model, proc = load(name, synthetic=1234)
    cfg = model.config
    for tensor, shape, row in (("model.layers.0.self_attn.q_proj.weight", (cfg.hidden, cfg.hidden), 3),
                               ("model.layers.0.mlp.gate_proj.weight", (cfg.ffn, cfg.hidden), 5)):
        t = model.read_tensor(tensor).reshape(shape).clone()
        t[row, 0], t[row, shape[1] // 2], t[row, shape[1] - 1] = 0.0, -0.0, 1e-40          # +0, -0 and a denormal
        model.load_tensor(tensor, t)
    enc = proc(images=sketch_image(0, 96), return_tensors="pt")
    ids, px = enc.input_ids[0], enc.pixel_values
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
        if w13:
            flagged = [model.lib.dtk_w13_flagged_rows(model._ctx, r) for r in range(5)]
            print(f"{name}: flagged rows q/k/v {flagged[0]}, o_proj {flagged[1]}, gate/up {flagged[2]}, down {flagged[3]}, lm_head {flagged[4]}")
            assert flagged[0] >= 1 and flagged[2] >= 1          # the general decode ran inside the captured step
    assert runs[0][0] == runs[1][0]
    for i, (a, b) in enumerate(zip(runs[0][1], runs[1][1])):
        assert np.array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32)), f"logits of step {i} differ"
    c1 = runs[1][2]["w13_counts"]
    assert (c1 & 1023, (c1 >> 10) & 1023, c1 >> 20) == (2 * cfg.layers + 1, 0, 0)


def test_flagged_rows_of_the_benchmarks_model():
    """the synthetic ds-7b of bench.py: every matrix still packs, and the rows that hold an exact zero (the generator draws on a 2^-23
    grid) are counted per role, not assumed"""
    from detikzify_amd.model import load
    model, _ = load("detikzify-ds-7b", synthetic=1234)
    model.set_option("w13", 1)
    us = C.c_float(0.0)
    model._check(model.lib.dtk_bench_gemv(model._ctx, 2, 0xFF, 1, C.byref(us)), "dtk_bench_gemv")
    c = model.stats()["w13_counts"]
    L, cfg = model.config.layers, model.config
    assert (c & 1023, (c >> 10) & 1023, c >> 20) == (3 * L + 1, 0, 0)
    rows = {"q/k/v": L * (cfg.hidden + 2 * cfg.num_kv_heads * cfg.head_dim), "o_proj": 0, "gate/up": L * 2 * cfg.ffn, "down": L * cfg.hidden, "lm_head": cfg.vocab}
    for r, (role, total) in enumerate(rows.items()):
        f = model.lib.dtk_w13_flagged_rows(model._ctx, r)
        print(f"ds-7b {role}: {f} of {total} packed rows hold a zero code")
        assert 0 <= f <= total
