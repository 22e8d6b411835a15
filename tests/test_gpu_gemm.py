"""The prefill GEMM family op by op on the MI355X, as the product calls it (dtk_op_gemm_ex): every case of tests/gemm_cases.py through
every kernel variant of a family — k_gemm_mfma per block tile x register stages x k-tile, k_gemm_glds, k_gemm_g3 tall / wide x row-major
/ fragment-major W x LDS / direct epilogue, the sliced-K pair, the in-register sliced kernel, the naive twin.  Per call: the launchers'
kernel record must equal the mirrored routing (a variant that silently fell through to another kernel fails here), the result is judged
against the float64 reference (grid classes: equality of bits; random: the bars of tests/gemm_cases.py), C starts as NaN poison with
NaN in every input gap and must keep every cell outside [M][N], the op itself fails if the guard bytes behind C were written.  Random
cases of the kernels that promise ONE k order are bit-equal to one fixed kernel's result (a module fixture: each family's test stands on
its own); every call is made a second time with another scratch poison byte, which must change nothing."""
from __future__ import annotations

import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest

from tests import gemm_cases as gc

pytestmark = pytest.mark.gpu

ERR_ARG = -1


@pytest.fixture(scope="module")
def tiny():
    """any context serves the op (it brings its own operands)"""
    from detikzify_amd.model import load
    return load("detikzify-tiny", synthetic=1234)[0]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@contextmanager
def options(m, opts):
    try:
        for k, v in opts.items():
            m.set_option(k, v)
        yield
    finally:
        for k in opts:
            m.set_option(k, gc.DEFAULTS[k])


def operands(c):
    if "_ops" not in c.__dict__:
        has_res = bool(c.flags & gc.RES) and not c.inplace
        c._ops = dict(A=c.a_buffer(), W=c.w_buffer(), bias=c.bias_buffer() if c.flags & gc.BIAS else None, res=c.res_buffer() if has_res else None,
                      gate=c.gate_buffer() if c.flags & gc.GATED else None)
    return c._ops


def call(m, c, v, fill=0xFF, **over):
    a = dict(operands(c), M=c.M, N=c.N, K=c.K, lda=c.lda, ldw=c.ldw, ldr=c.ldr, ldc=c.ldc, b_off=c.b_off, r_off=c.r_off, c_off=c.c_off,
             flags=c.flags | v.flags | (c.S << gc.KS_SHIFT), buf=c.initial())
    a.update(over)
    n = lambda x: 0 if x is None else x.size
    sizes = dict(na=n(a["A"]), nw=n(a["W"]), nb=n(a["bias"]), nr=n(a["res"]), nc=n(a["buf"]))
    sizes.update({k: over[k] for k in sizes if k in over})
    code = C.c_int(-1)
    rc = m.lib.dtk_op_gemm_ex(m._ctx, _p(a["A"]), sizes["na"], _p(a["W"]), sizes["nw"], _p(a["bias"]), sizes["nb"], _p(a["res"]), sizes["nr"], _p(a["gate"]),
                              _p(a["buf"]), sizes["nc"], a["M"], a["N"], a["K"], a["lda"], a["ldw"], a["ldr"], a["ldc"], a["b_off"], a["r_off"], a["c_off"],
                              a["flags"], fill, C.byref(code))
    return rc, a["buf"], code.value


def run(m, c, v, fill=0xFF):
    rc, buf, code = call(m, c, v, fill)
    m._check(rc, f"{c.name} {v.name}")
    return buf, code


@pytest.fixture(scope="module")
def anchor_bits(tiny):
    """random case -> its C buffer from ONE fixed kernel (gemm_cases.anchor: k_gemm_mfma 64 x 64 D = 3, or the tall row-major sliced-K pair):
    what every kernel that promises the same k order must reproduce bit for bit, whichever families a run selects"""
    out = {}
    for c in gc.all_cases():
        if c.kind != "exact":
            v = gc.anchor(c)
            with options(tiny, v.opts):
                out[c.name], code = run(tiny, c, v)
            assert code == gc.route(c, v), (c.name, hex(code))
    return out


@pytest.mark.parametrize("family", gc.ONE_CHAIN_FAMILIES + ("sk", "sl"))
def test_gemm_family(tiny, anchor_bits, family):
    ws, wc, ran = (0.0, 0.0, 0.0), (0.0, 0.0), 0
    for v in gc.variants(family):
        with options(tiny, v.opts):
            for c in gc.cases_of(family):
                buf, code = run(tiny, c, v)
                want = gc.route(c, v)
                assert code == want, f"{c.name} {v.name}: kernel record {code:#x}, the routing says {want:#x}"
                ok, fig = c.judge(buf)
                if not ok:
                    print(f"{c.name} {v.name}: {fig}")
                assert ok, (c.name, v.name, fig)
                ran += 1
                if c.kind != "exact":
                    ws, wc = tuple(map(max, ws, fig["single"])), tuple(map(max, wc, fig["chain"]))
                    if family != "naive":       # (the naive twin's fmaf chain is another order inside a 32-wide k-step)
                        assert np.array_equal(anchor_bits[c.name], buf), f"{c.name} {v.name}: not the bits of {gc.anchor(c).name}"
                again, _ = run(tiny, c, v, fill=0x00)
                assert np.array_equal(again, buf), f"{c.name} {v.name}: the scratch poison shows in the result"
    print(f"{family}: {ran} calls, every grid / GELU-grid / order case bit-equal to float64; random single-rounding differing {ws[0]:.4f} max_ulp {ws[1]:.2f} "
          f"rel_l2 {ws[2]:.2e}; random chained max_ulp {wc[0]:.2f} rel_l2 {wc[1]:.2e}")


def test_gemm_ex_refusals(tiny):
    """what the product never hands a GEMM is DTK_ERR_ARG with nothing launched and C untouched; the stride errors name the operand"""
    v, sk, sl = gc.variants("default")[0], gc.variants("sk")[0], gc.variants("sl")[0]
    c = next(x for x in gc.one_chain_cases() if x.tag == "align" and x.epi == "bias_res" and x.pat == gc.PAT[0] and x.N == 136)
    s = next(x for x in gc.sliced_cases() if x.cls == "grid" and x.K == 200 and x.S == 2)
    short = next(x for x in gc.one_chain_cases() if x.K == 72 and x.cls == "grid")
    bad = [(c, v, dict(lda=c.lda + 4), "lda"), (c, v, dict(ldw=c.ldw - 4), "ldw"), (c, v, dict(lda=c.K - 8), "lda"), (c, v, dict(na=c.M * c.lda - c.lda), " A "),
           (c, v, dict(nw=c.N * c.ldw - c.ldw), " W "), (c, v, dict(nb=c.N - 1), "bias"), (c, v, dict(nr=c.M * c.ldr - c.ldr), "residual"),
           (c, v, dict(nc=c.M * c.ldc - 1), " C "), (c, v, dict(ldc=c.N - 8), "ldc"), (c, v, dict(c_off=8), " C "), (c, v, dict(r_off=16), "residual"),
           (c, v, dict(b_off=1), "bias"), (c, v, dict(K=c.K + 4), "K"), (c, v, dict(flags=c.flags | (9 << gc.KS_SHIFT)), "8 K slices"),
           (c, v, dict(flags=c.flags | gc.INPLACE), "INPLACE"), (c, v, dict(flags=c.flags | gc.GATED), "gate"), (c, v, dict(res=None), "residual"),
           (s, sl, dict(flags=s.flags | gc.SL | (1 << gc.KS_SHIFT)), "SL"), (short, sk, dict(flags=short.flags | (2 << gc.KS_SHIFT)), "sliced")]
    for case, var, over, word in bad:
        rc, buf, _ = call(tiny, case, var, **over)
        msg = tiny.lib.dtk_last_error(tiny._ctx).decode()
        assert rc == ERR_ARG, (case.name, over, rc)
        assert word in msg, (over, msg)
        assert np.array_equal(buf, case.initial()), (case.name, over)
    for case, var in ((c, v), (s, sk), (s, sl)):          # the same calls without the fault are taken
        buf, _ = run(tiny, case, var)
        ok, fig = case.judge(buf)
        assert ok, (case.name, fig)
