"""The weight kernels of the batched decode step op by op on the MI355X (dtk_op_gemv_b / dtk_op_gemv_bkp) against the float64
reference of tests/gemv_b_cases.py: k_gemv_b in every shape launch_gemv_b_impl can pick, the 64-slot kernels k_gemv_bx / bl (and its
Q3 qkv form) / br / bc / bus, the K-slice pair k_gemv_bkp | k_gemv_bkl + k_resid_norm_b, and with them k_rmsnorm_b, k_retile and
k_retile_f8.  Every buffer starts as NaN poison; what a role must not write has to keep its bits, idle slots included.

The launchers are not instrumented, and a launcher that declines has no observable effect: the dispatcher goes on to the next kernel
and in the end to k_gemv_b.  So a fall-through is ACCEPTED here, not noticed.  Each run carries a label with the kernel its options ask
for (it appears in the assertion messages and in the printed worst figures, not in the test ids); the result is held to the float64
bars whichever kernel ran, and — the source's promise (csrc/kernels.h) — to bit equality with k_gemv_b's result of the same run, which
says something on the random-operand cases only (on GRID operands every order gives the same sums).  Where the code says a launcher
declines, the label says "(declines: why)" and the run covers the dispatcher's way past it.  Silent refusals a label cannot foresee:
k_gemv_br, k_gemv_bc and k_gemv_bus decline when the compiler gave the instantiation scratch memory or the LDS attribute cannot be set
(br_usable / bc_usable / bus_usable), k_gemv_bx / k_gemv_bl / k_gemv_br for more than 4 units per block (not at these shapes).
Unreachable at these shapes: see the docstring of tests/gemv_b_cases.py."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from oracle.ops import f32_to_bits
from tests import gemv_b_cases as gc

pytestmark = pytest.mark.gpu

DEFAULTS = {"gemv_bx": 1, "resid_split": 1, "gemv_b_wide": 2, "gemv_bl": 33, "gemv_bkl": 1, "gemv_xw": 0, "gemv_loaders": 1, "gemv_br_wd": 4,
            "gemv_bc": 128, "gemv_bus": 128}
PLAIN = {"gemv_bx": 0, "gemv_bl": 0, "gemv_bc": 0, "gemv_bus": 0, "gemv_xw": 0, "gemv_loaders": 1, "gemv_br_wd": 4}      # k_gemv_b alone


@pytest.fixture(scope="module")
def tiny():
    from detikzify_amd.model import load
    return load("detikzify-tiny", synthetic=1234)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _set(model, **opts):
    for k, v in opts.items():
        model.set_option(k, v)


def _operands(case):
    if not hasattr(case, "dev"):
        case.dev = dict(W=None if case.fmt == "fp8" else f32_to_bits(case.W), W8=case.W8,
                        ws=case.wscale.numpy().astype(np.float32) if case.fmt == "fp8" else None,
                        X=f32_to_bits(case.X), nw=f32_to_bits(case.norm_w), pos=np.asarray(case.pos, dtype=np.int32))
        if case.epi == gc.QKV:
            case.dev.update(cos=f32_to_bits(case.cos), sin=f32_to_bits(case.sin))
    return case.dev


def _run(model, case, nslots, active):
    """one dtk_op_gemv_b call on poisoned buffers; returns the buffers"""
    o, buf = _operands(case), case.initial(active)
    act = np.asarray(active, dtype=np.int32)
    err = np.full(1, 0xFFFFFFFF, dtype=np.uint32)
    g = lambda n: _p(buf.get(n))
    model._check(model.lib.dtk_op_gemv_b(
        model._ctx, case.epi, _p(o["W"]), _p(o["W8"]), _p(o["ws"]), case.N, case.K, _p(np.ascontiguousarray(o["X"][:nslots])),
        _p(o["nw"]) if case.norm else None, gc.EPS, _p(act), _p(o["pos"]), nslots, case.d, case.ff, case.H, case.KVH, gc.T_MAX,
        _p(o.get("cos")), _p(o.get("sin")), g("q"), g("k"), g("v"), g("y"), g("frag"), g("logits"), None, _p(err)), "dtk_op_gemv_b")
    assert err[0] == 0, f"{case.name}: {err[0]} expired hand-off waits"
    return buf


class Worst:
    def __init__(self):
        self.w = {}

    def add(self, name, fig):
        s, c = self.w.get(name, ((0.0, 0.0, 0.0), (0.0, 0.0)))
        self.w[name] = (tuple(map(max, s, fig["single"])), tuple(map(max, c, fig["chain"])))

    def show(self):
        for name, (s, c) in self.w.items():
            print(f"{name}: single-rounding differing {s[0]:.4f} max_ulp {s[1]:.2f} rel_l2 {s[2]:.2e}; chained max_ulp {c[0]:.2f} rel_l2 {c[1]:.2e}")


def _check(model, case, nslots, layout, active, label, worst, family):
    buf = _run(model, case, nslots, active)
    ok, fig = case.judge(buf, active)
    if not ok:
        print(f"{label} {case.name} nslots {nslots} {layout}: {fig}")
    if fig["single"][0] == fig["single"][0] and fig["chain"][0] == fig["chain"][0]:
        worst.add(family, fig)
    assert ok, f"{label} {case.name} nslots {nslots} {layout}: {fig}"
    return buf


def _same(a, b):
    return all(np.array_equal(a[n].view(np.uint8), b[n].view(np.uint8)) for n in a)


# ------------------------------------------------------------------------------------------ k_gemv_b
@pytest.mark.parametrize("epi", [gc.STORE, gc.RESID, gc.QKV, gc.SWIGLU, gc.LOGITS], ids=lambda e: gc.EPI_NAME[e])
def test_k_gemv_b_every_instantiation(tiny, epi):
    """special kernels off: NT = 1 / 2 / 4 (nslots 1, 16, 17, 32, 33, 64) x gemv_b_wide 0 / 1 / 3 / 6 (x resid_split for RESID) x bf16 / fp8
    x K 40 / 72 / 256 / 304 at ragged N; a row's k order depends on the wave split of K only, so the 8-wave modes (0, 1, 6, either
    resid_split) must agree bit for bit"""
    model, _ = tiny
    worst = Worst()
    try:
        _set(model, **PLAIN)
        for case in (c for c in gc.small_cases() if c.epi == epi):
            for nslots, layout, active in gc.runs(case):
                base = None
                for split in ((0, 1) if epi == gc.RESID else (1,)):
                    for wide in gc.WIDE:
                        _set(model, gemv_b_wide=wide, resid_split=split)
                        buf = _check(model, case, nslots, layout, active, f"k_gemv_b wide {wide} resid_split {split}", worst,
                                     f"k_gemv_b {gc.EPI_NAME[epi]} {case.fmt}" + (" GRID" if case.grid else ""))
                        if wide != 3:       # (mode 3 splits K over 4 waves instead of 8: other chains, the same bars)
                            base = base or buf
                            assert _same(buf, base), f"{case.name} nslots {nslots} {layout}: gemv_b_wide {wide} resid_split {split} changes bits"
    finally:
        _set(model, **DEFAULTS)
    worst.show()


# ------------------------------------------------------------------------------------------ the 64-slot kernels
def _variants(case):
    """(label, options) of the 64-slot kernels that can take the case; `declines` = the launcher refuses it and k_gemv_b serves"""
    f8, qkv, K = case.fmt == "fp8", case.epi == gc.QKV, case.K
    mha = qkv and case.H == case.KVH
    out = []
    if K == 2048:
        out += [(f"k_gemv_bx units {u}", dict(gemv_bx=u)) for u in (2, 3, 4)]
        out += [("k_gemv_bx auto (declines: fewer than 3 units per CU)", dict(gemv_bx=1))]
        bl = (2 if qkv else 1) | (4 if f8 else 0)
        out += [(f"k_gemv_bl {bl} xw {xw}", dict(gemv_bl=bl, gemv_xw=xw)) for xw in (0, 1, 2)]
        if f8:
            out += [(f"k_gemv_bl {bl & 3} (declines: fp8 without bit 2)", dict(gemv_bl=bl & 3))]
        if qkv:
            for bit in (8, 16):
                for loaders in (1, 2):
                    for xw in (0, 1, 2):
                        name = "k_gemv_bl Q3" if (bit == 16 and mha) else "k_gemv_bl Q3 (declines: " + ("GQA)" if not mha else "too few pairs for bit 3)")
                        out += [(f"{name} bit {bit} loaders {loaders} xw {xw}", dict(gemv_bl=bit | (4 if f8 else 0), gemv_loaders=loaders, gemv_xw=xw))]
        out += [(f"k_gemv_bc units {u}", dict(gemv_bc=7 | (u << 4))) for u in (0, 1, 2, 3, 4)]
        role_bit = {gc.QKV: 1, gc.SWIGLU: 2, gc.LOGITS: 0}[case.epi]
        out += [(f"k_gemv_bus {v}" if v & role_bit else f"k_gemv_bus (declines: option {v} leaves the role out)", dict(gemv_bus=v)) for v in (1, 2, 3)]
    else:       # K = 4096: k_gemv_br (fp8 weights by bit 5, bf16 qkv by bit 6)
        if f8:
            out += [(f"k_gemv_br fp8 wd {wd}", dict(gemv_bl=32, gemv_br_wd=wd)) for wd in (4, 8)]
        elif qkv:
            out += [("k_gemv_br bf16 qkv", dict(gemv_bl=64))]
        else:
            out += [("k_gemv_br (declines: bf16 gate/up, lm_head)", dict(gemv_bl=64))]
        out += [("k_gemv_bx units 2 (K 4096)", dict(gemv_bx=2)), ("k_gemv_bc units 1 (K 4096)", dict(gemv_bc=7 | 16))]
        if case.epi != gc.LOGITS:
            out += [("k_gemv_bus 3 (K 4096)", dict(gemv_bus=3))]
    return out


@pytest.mark.parametrize("K", [2048, 4096])
@pytest.mark.parametrize("epi", [gc.QKV, gc.SWIGLU, gc.LOGITS], ids=lambda e: gc.EPI_NAME[e])
def test_64_slot_kernels(tiny, epi, K):
    """nslots 49 and 64 (their gate is nt >= 3); qkv at H/KVH 2/1 and 2/2, gate/up at ff 80 / 96, lm_head at N 160 / 192: five row-tile
    groups leave surplus waves in the last block at 2, 3 and 4 units per block.  Every shape on GRID operands (equality with the float64
    reference) and on random ones (the bars of LOGITS, V, SwiGLU, q / k), every result equal to k_gemv_b's bit for bit — on the random
    operands a kernel that summed in another order, in the last block alone even, would differ"""
    model, _ = tiny
    worst = Worst()
    try:
        for case in (c for c in gc.big_cases(K) if c.epi == epi):
            for nslots, layout, active in gc.runs(case):
                _set(model, **PLAIN)
                _set(model, gemv_b_wide=0)
                base = _check(model, case, nslots, layout, active, "k_gemv_b", worst,
                              f"k_gemv_b {gc.EPI_NAME[epi]} K {K}" + (" GRID" if case.grid else " random"))
                for label, opts in _variants(case):
                    _set(model, **PLAIN)
                    _set(model, **opts)
                    buf = _check(model, case, nslots, layout, active, label, worst,
                                 label.split(" (")[0].split(" units")[0].split(" xw")[0] + (" GRID" if case.grid else " random"))
                    assert _same(buf, base), f"{label} {case.name} nslots {nslots} {layout}: not k_gemv_b's bits"
    finally:
        _set(model, **DEFAULTS)
    worst.show()


# ------------------------------------------------------------------------------------------ k_gemv_bkp / k_gemv_bkl + k_resid_norm_b
def _run_bkp(model, case, nslots, active, K=None, expect_refusal=False):
    o, buf = _operands(case), case.initial(active)
    act = np.asarray(active, dtype=np.int32)
    K = K or case.K
    part = np.full((8, gc.SLOTS, case.N), np.float32(-7.0), dtype=np.float32)
    err = np.full(1, 0xFFFFFFFF, dtype=np.uint32)
    W = None if o["W"] is None else np.ascontiguousarray(o["W"][:, :K])
    W8 = None if o["W8"] is None else np.ascontiguousarray(o["W8"][:, :K])
    rc = model.lib.dtk_op_gemv_bkp(model._ctx, _p(W), _p(W8), _p(o["ws"]), case.N, K, _p(np.ascontiguousarray(o["X"][:nslots, :K])), _p(act), nslots,
                                   _p(o["nw"]), gc.EPS, _p(buf["y"]), _p(buf["xn"]), _p(part), _p(err))
    if expect_refusal:
        return rc, buf, part, err
    model._check(rc, "dtk_op_gemv_bkp")
    assert err[0] == 0, f"{case.name}: {err[0]} expired hand-off waits"
    return buf, part


def _two_launch_twin(model, case, nslots, active):
    """the same operands through dtk_op_gemv_b(RESID), then k_rmsnorm_b on the updated rows (the prologue of a STORE role)"""
    o, buf = _operands(case), case.initial(active)
    act = np.asarray(active, dtype=np.int32)
    err = np.zeros(1, dtype=np.uint32)
    model._check(model.lib.dtk_op_gemv_b(
        model._ctx, gc.RESID, _p(o["W"]), _p(o["W8"]), _p(o["ws"]), case.N, case.K, _p(np.ascontiguousarray(o["X"][:nslots])), None, gc.EPS,
        _p(act), None, nslots, case.K, 0, 0, 0, 0, None, None, None, None, None, _p(buf["y"]), None, None, None, _p(err)), "dtk_op_gemv_b")
    assert err[0] == 0
    w16 = np.zeros((16, case.N), dtype=np.uint16)
    y16 = np.zeros((gc.SLOTS, 16), dtype=np.uint16)
    xn = np.zeros((nslots, case.N), dtype=np.uint16)
    resid = np.ascontiguousarray(buf["y"][:nslots]).copy()
    resid[np.asarray(active) == 0] = 0          # (idle rows are NaN poison here; k_rmsnorm_b skips them)
    model._check(model.lib.dtk_op_gemv_b(
        model._ctx, gc.STORE, _p(w16), None, None, 16, case.N, _p(resid), _p(o["nw"]), gc.EPS, _p(act), None, nslots, case.N, 0, 0, 0, 0,
        None, None, None, None, None, _p(y16), None, None, _p(xn), _p(err)), "dtk_op_gemv_b")
    return buf["y"], xn


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("N,K", gc.BKP_SHAPES)
def test_k_slice_pair(tiny, N, K, fmt):
    """N 2048 (4 row tiles per block, one round of k_resid_norm_b) and 4096 (8, two rounds) x K 256 / 480 / 768 (one k-step per slice,
    a one-step last slice, slices that start at odd k-steps) x gemv_bkl 0 / 1 x gemv_xw 0..2, 33 and 64 slots with idle ones: the sum of the
    eight partial planes, the residual, the normalised rows; bit-identical to k_gemv_b<RESID> + k_rmsnorm_b"""
    model, _ = tiny
    worst = Worst()
    cases = [c for c in gc.bkp_cases() if (c.N, c.K, c.fmt) == (N, K, fmt)]
    assert cases and all(c.grid for c in cases[1:])
    try:
        for case in cases:
            for nslots, layout, active in gc.runs(case):
                _set(model, **PLAIN)
                _set(model, gemv_b_wide=0, resid_split=1)
                y_twin, xn_twin = _two_launch_twin(model, case, nslots, active)
                for bkl in ((1,) if fmt == "fp8" else (0, 1)):            # fp8 weights: only the LDS-ring kernel reads the pair tiles
                    for xw in ((0, 1, 2) if bkl else (0,)):
                        _set(model, gemv_bkl=bkl, gemv_xw=xw)
                        label = f"{'k_gemv_bkl' if bkl else 'k_gemv_bkp'} xw {xw}"
                        buf, part = _run_bkp(model, case, nslots, active)
                        ok, fig = case.judge(buf, active, partial_sum=part.astype(np.float64).sum(0))
                        if fig["chain"][0] == fig["chain"][0]:
                            worst.add(label.split(" xw")[0] + " + k_resid_norm_b", fig)
                        assert ok, f"{label} {case.name} nslots {nslots} {layout}: {fig}"
                        rows = [s for s, a in enumerate(active) if a]
                        assert np.array_equal(buf["y"], y_twin), f"{label} {case.name} nslots {nslots} {layout}: residual differs from k_gemv_b<RESID>"
                        assert np.array_equal(buf["xn"][rows], xn_twin[rows]), f"{label} {case.name} nslots {nslots} {layout}: norm differs from k_rmsnorm_b"
    finally:
        _set(model, **DEFAULTS)
    worst.show()


def test_swiglu_refuses_a_width_the_context_would_refuse(tiny):
    """ff % 8 != 0: dtk_create does not take such a model, and the op does not either"""
    from detikzify_amd._lib import DtkError
    model, _ = tiny
    case = gc._case(gc.SWIGLU, "bf16", 40, ff=24)
    case.ff, case.N = 20, 40
    try:
        with pytest.raises(DtkError):
            _run(model, case, 16, gc.active_sets(16)["interleaved"])
    finally:
        case.ff, case.N = 24, 48


def test_k_slice_pair_refuses_what_the_step_would_not_give_it(tiny):
    """K = 448: 14 k-steps, two per slice, the eighth slice empty; 32 slots; fp8 weights with gemv_bkl 0 — DTK_ERR_ARG, nothing written"""
    model, _ = tiny
    try:
        _set(model, **PLAIN)
        for case, nslots, K, bkl in ((gc._case(gc.BKP, "bf16", 480, N=2048), 64, 448, 1), (gc._case(gc.BKP, "bf16", 480, N=2048), 64, 448, 0),
                                     (gc._case(gc.BKP, "bf16", 256, N=2048), 32, 256, 1), (gc._case(gc.BKP, "fp8", 256, N=2048), 64, 256, 0)):
            _set(model, gemv_bkl=bkl)
            active = gc.active_sets(nslots)["interleaved"]
            rc, buf, part, err = _run_bkp(model, case, nslots, active, K=K, expect_refusal=True)
            init = case.initial(active)
            assert rc == -1 and "not covered" in model.lib.dtk_last_error(model._ctx).decode()
            assert all(np.array_equal(buf[n], init[n]) for n in init) and (part == np.float32(-7.0)).all() and err[0] == 0xFFFFFFFF
    finally:
        _set(model, **DEFAULTS)
