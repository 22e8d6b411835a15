"""The weight kernel of the single-sequence decode step, k_gemv, op by op on the MI355X (dtk_op_gemv_role) against the float64
reference of tests/gemv_cases.py: every (prologue, epilogue, weight format) the step has, in every shape of launch_gemv_variant,
launch_gemv_f8_variant and launch_gemv_q4.  Every result buffer starts as NaN poison and the op's device scratch as 0xFF bytes (NaN
in every format a kernel might read beside its operands); what a role must not write has to keep its bits, and the op itself fails
if anything behind the end of a result buffer was written.

Besides the bars: gemv_inl.h promises that a lane folds chunks lane, lane + 64, ... of its row in that order whatever U is, so on
random operands all KS = 1 variants of a role and format must agree bit for bit whatever R, U, persistence and grid (under
PRO_RMSNORM among variants of equal wave count: the norm's own reduction follows the block size); a split-K variant must agree
with itself under another scratch poison (its merge is fixed-order); variant -1 must be the variant launch_gemv's table names."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from oracle.ops import f32_to_bits
from tests import gemv_cases as gc

pytestmark = pytest.mark.gpu

ROLE_ID = lambda r: f"{gc.PRO_NAME[r[0]]}-{gc.EPI_NAME[r[1]]}-{r[2]}"
ERR_ARG = -1


@pytest.fixture(scope="module")
def tiny():
    """any context serves the op (it brings its own weights)"""
    from detikzify_amd.model import load
    return load("detikzify-tiny", synthetic=1234)[0]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _operands(case):
    if not hasattr(case, "dev"):
        f32 = lambda t: np.ascontiguousarray(t.numpy().astype(np.float32))
        o = dict(W=f32_to_bits(case.W) if case.fmt == "bf16" else None, W8=case.W8, ws=f32(case.wscale) if case.fmt == "fp8" else None,
                 W4=case.W4, S4=case.S4, x=None, nw=None, cos=None, sin=None, pm=None, pl=None, po=None)
        if case.pro == gc.ATTN:
            o.update(pm=f32(case.pm), pl=f32(case.pl), po=f32(case.po))
        else:
            o["x"] = f32_to_bits(case.x)
        if case.pro == gc.RMSNORM:
            o["nw"] = f32_to_bits(case.norm_w)
        if case.epi == gc.QKV:
            o.update(cos=f32_to_bits(case.cos), sin=f32_to_bits(case.sin))
        case.dev = o
    return case.dev


def _call(model, case, variant, d=0, fill=0xFF, **over):
    """one dtk_op_gemv_role call on poisoned buffers; returns (rc, buffers).  `over` replaces arguments by name (the refusals)."""
    o, buf = _operands(case), case.initial()
    a = dict(pro=case.pro, epi=case.epi, variant=variant, W=o["W"], W8=o["W8"], ws=o["ws"], W4=o["W4"], S4=o["S4"], N=case.N, K=case.K,
             d=case.d if case.epi == gc.QKV else d, ff=case.ff, H=case.H, KVH=case.KVH, hd=case.hd, T_max=gc.T_MAX, pos=case.pos, S=case.S)
    a.update(over)
    g = lambda n: _p(buf.get(n))
    rc = model.lib.dtk_op_gemv_role(model._ctx, a["pro"], a["epi"], a["variant"], _p(a["W"]), _p(a["W8"]), _p(a["ws"]), _p(a["W4"]), _p(a["S4"]),
                                    a["N"], a["K"], a["d"], a["ff"], a["H"], a["KVH"], a["hd"], a["T_max"], a["pos"], gc.EPS,
                                    _p(o["x"]), _p(o["nw"]), _p(o["cos"]), _p(o["sin"]), a["S"], _p(o["pm"]), _p(o["pl"]), _p(o["po"]), fill,
                                    g("q"), g("k"), g("v"), g("y"), g("logits"))
    return rc, buf


def _run(model, case, variant, d=0, fill=0xFF):
    rc, buf = _call(model, case, variant, d, fill)
    model._check(rc, f"dtk_op_gemv_role {case.name} variant {variant}")
    return buf


def _same(a, b):
    return all(np.array_equal(a[n].view(np.uint8), b[n].view(np.uint8)) for n in a)


class Worst:
    def __init__(self):
        self.w = {}

    def add(self, name, fig):
        s, c = self.w.get(name, ((0.0, 0.0, 0.0), (0.0, 0.0)))
        self.w[name] = (tuple(map(max, s, fig["single"])), tuple(map(max, c, fig["chain"])))

    def show(self):
        for name, (s, c) in self.w.items():
            print(f"{name}: single-rounding differing {s[0]:.4f} max_ulp {s[1]:.2f} rel_l2 {s[2]:.2e}; chained max_ulp {c[0]:.2f} rel_l2 {c[1]:.2e}")


def _judged(model, case, variant, worst, group, d=0, fill=0xFF):
    buf = _run(model, case, variant, d, fill)
    ok, fig = case.judge(buf)
    if fig["single"][0] == fig["single"][0] and fig["chain"][0] == fig["chain"][0]:
        worst.add(group, fig)
    assert ok, f"{case.name} variant {variant} d {d}: {fig}"
    return buf


def _group(role, v):
    """the variants that must agree bit for bit share a group: KS = 1 (under PRO_RMSNORM: of one wave count); a split-K variant is alone"""
    R, U, waves, bpc, KS = gc.TABLE[role][v]
    if KS > 1:
        return f"split-K {KS} variant {v}"
    return f"KS 1, {waves} waves" if role[0] == gc.RMSNORM else "KS 1"


# ------------------------------------------------------------------------------------------ every role x format x variant
@pytest.mark.parametrize("role", gc.ROLES, ids=ROLE_ID)
def test_every_variant_against_float64(tiny, role):
    pro, epi, fmt = role
    worst = Worst()
    for case in gc.role_cases(*role):
        kind = " GRID" if case.grid else ""
        base, got = {}, {}
        for v in case.variants():
            grp = _group(role, v)
            buf = got[v] = _judged(tiny, case, v, worst, f"{ROLE_ID(role)} {grp}{kind}")
            if gc.TABLE[role][v][4] > 1:      # split-K: the merge in LDS is fixed-order, so another scratch poison changes nothing
                again = _judged(tiny, case, v, worst, f"{ROLE_ID(role)} {grp}{kind}", fill=0x5A)
                assert _same(again, buf), f"{case.name} variant {v}: two runs differ"
            else:
                base.setdefault(grp, (v, buf))
                assert _same(buf, base[grp][1]), f"{case.name}: variant {v} and variant {base[grp][0]} ({grp}) differ in bits"
        if fmt == "mxfp4":
            continue                          # (-1 is the only variant)
        for d in ((case.d,) if epi == gc.QKV else (2048, 4096)):
            want = gc.default_variant(pro, epi, fmt, case.K, d)
            buf = _judged(tiny, case, -1, worst, f"{ROLE_ID(role)} default{kind}", d=d)
            assert _same(buf, got[want]), f"{case.name}: variant -1 at d {d} is not variant {want}"
    worst.show()


# ------------------------------------------------------------------------------------------ the second trip of a persistent wave
@pytest.mark.parametrize("fmt", ["bf16", "fp8", "mxfp4"])
def test_persistent_second_trip(tiny, fmt):
    """K = 64 and more units than CUs x blocks per CU x waves x R by less than one round: some waves set their rows again, load their
    first stage and prefetch the next chunk's epilogue operands while this chunk's are still to be used; the others stop"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    worst = Worst()
    for pro, epi, f, v in (s for s in gc.persistent_shapes() if s[2] == fmt):
        role = (pro, epi, f)
        R, U, waves, bpc, KS = gc.TABLE[role][v]
        for hd in ((128, 64) if epi == gc.QKV else (128,)):
            case, first = gc.persistent_case(pro, epi, f, v, hd, cus)
            assert first == cus * bpc * waves * R and first < case.units < 2 * first, (case.name, cus, first, case.units)
            buf = _judged(tiny, case, v, worst, f"{ROLE_ID(role)} persistent")
            twin = [t for t, s in sorted(gc.TABLE[role].items()) if not s[3] and s[4] == 1 and (pro != gc.RMSNORM or s[2] == waves)]
            if twin:      # one chunk per wave, the same sums
                assert _same(_judged(tiny, case, twin[0], worst, f"{ROLE_ID(role)} persistent"), buf), f"{case.name}: variant {v} and variant {twin[0]} differ in bits"
    worst.show()


# ------------------------------------------------------------------------------------------ EPI_STORE = dtk_op_gemv / dtk_op_gemv_q4
@pytest.mark.parametrize("fmt", ["bf16", "mxfp4"])
def test_store_equals_dtk_op_gemv(tiny, fmt):
    for pro in (gc.COPY, gc.RMSNORM):
        for case in gc.role_cases(pro, gc.STORE, fmt):
            o = _operands(case)
            y = np.full(case.N, gc.NAN_Y, dtype=np.uint16)
            nw = o["nw"] if pro == gc.RMSNORM else np.zeros(case.K, dtype=np.uint16)
            Wb = f32_to_bits(case.W)
            if fmt == "bf16":
                tiny._check(tiny.lib.dtk_op_gemv(tiny._ctx, _p(Wb), _p(o["x"]), _p(nw), case.N, case.K, int(pro == gc.RMSNORM), gc.EPS, _p(y)), "dtk_op_gemv")
            else:     # the de-quantised weights quantise to themselves in value
                tiny._check(tiny.lib.dtk_op_gemv_q4(tiny._ctx, _p(Wb), _p(o["x"]), _p(nw), case.N, case.K, int(pro == gc.RMSNORM), gc.EPS, _p(y), None), "dtk_op_gemv_q4")
            assert np.array_equal(_run(tiny, case, -1)["y"], y), case.name


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_touch_nothing(tiny):
    """everything the step would never hand these kernels: DTK_ERR_ARG, nothing launched, every buffer as it was"""
    qkv = gc._case(gc.RMSNORM, gc.QKV, "bf16", 72, H=2, KVH=1, hd=64, pos=gc.POS_IN)
    qkv8 = gc._case(gc.RMSNORM, gc.QKV, "fp8", 1040, H=2, KVH=1, hd=64, pos=gc.POS_IN)
    swi = gc._case(gc.RMSNORM, gc.SWIGLU, "bf16", 72, ff=24)
    res = gc._case(gc.COPY, gc.RESID, "bf16", 72, N=37)
    res8 = gc._case(gc.COPY, gc.RESID, "fp8", 1040, N=37)
    res4 = gc._case(gc.COPY, gc.RESID, "mxfp4", 72, N=37)
    att = gc._case(gc.ATTN, gc.RESID, "bf16", H=2, hd=128, S=3, N=37)
    log = gc._case(gc.RMSNORM, gc.LOGITS, "bf16", 72, N=37)
    sto = gc._case(gc.COPY, gc.STORE, "bf16", 72, N=37)
    bad = [(res, -1, dict(K=76)), (res, -1, dict(K=0)), (res8, -1, dict(K=1032)), (res4, -1, dict(K=76)),
           (swi, -1, dict(ff=20, N=40)), (swi, -1, dict(N=40)), (swi, -1, dict(ff=0, N=0)),
           (qkv, -1, dict(N=qkv.N - 64)), (qkv, -1, dict(KVH=2)), (qkv, -1, dict(H=3, KVH=2, N=7 * 64, d=3 * 64)), (qkv, -1, dict(hd=32)),
           (qkv, -1, dict(hd=96)), (qkv, -1, dict(pos=-1)), (qkv, -1, dict(pos=gc.T_MAX)), (qkv8, -1, dict(pos=gc.T_MAX)),
           (att, -1, dict(S=0)), (att, -1, dict(S=17)), (att, -1, dict(hd=32)), (att, -1, dict(K=att.K - 8)),
           # a (prologue, epilogue) pair without a kernel in the format (launch_gemv_q4 would abort the process; the others would run another role)
           (res4, -1, dict(epi=gc.LOGITS)), (res4, -1, dict(pro=gc.RMSNORM, epi=gc.RESID)), (res8, -1, dict(epi=gc.STORE)),
           (res8, -1, dict(pro=gc.RMSNORM)), (res, -1, dict(pro=gc.RMSNORM)), (log, -1, dict(pro=gc.COPY)), (swi, -1, dict(pro=gc.COPY)),
           (qkv, -1, dict(pro=gc.COPY)), (att, -1, dict(epi=gc.STORE)), (res, -1, dict(pro=3)), (res, -1, dict(epi=5)), (res, -1, dict(epi=-1)),
           # a variant outside the table
           (res, 23, {}), (res, -2, {}), (att, 9, {}), (log, 5, {}), (qkv, 12, {}), (swi, 12, {}), (sto, 1, {}), (sto, 22, {}),
           (res8, 10, {}), (qkv8, 10, {}), (res4, 0, {}),
           # not exactly one weight operand
           (res, -1, dict(W=None)), (res8, -1, dict(ws=None)), (res4, -1, dict(S4=None)), (res, -1, dict(W8=res8.W8, ws=np.ones(37, dtype=np.float32)))]
    for case, variant, over in bad:
        rc, buf = _call(tiny, case, variant, **over)
        init = case.initial()
        assert rc == ERR_ARG, (case.name, variant, over.keys(), rc)
        assert all(np.array_equal(buf[n].view(np.uint8), init[n].view(np.uint8)) for n in init), (case.name, variant, list(over))
    # (and the same calls without the fault are taken)
    for case in (qkv, qkv8, swi, res, res8, res4, att, log, sto):
        assert case.judge(_run(tiny, case, -1))[0], case.name
