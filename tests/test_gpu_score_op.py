"""The scoring head op by op on the MI355X (dtk_op_score / dtk_op_score_top): every case of tests/score_cases.py through the log-softmax
epilogue of k_gemm_mfma<64, 128> or k_gemm_g3 (tall / wide, row-major and fragment-major W), k_score_merge and k_score_top.  Per call:
argmax, zmax, top_ids, top_z bit-equal to the float64 reference of the operands; |lse - ref| <= 2e-5; logprob and top_logprob bit-equal
to the ONE fp32 subtraction of the device's lse from the reference's z; everything finite; the launcher's kernel record equals the
mirrored routing; the outputs start as NaN / sentinel poison with a tail the call does not own, the op's scratch starts as 0xFF (a
record left out is NaN) and its guard bytes must survive (the op fails otherwise); every call is made twice and must reproduce its
bits.  A row's outputs are the same bits with W as fragment-major tiles, for every k, as the only row of a call, and under the other
tile orientation."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from oracle.ops import bits_to_f32, f32_to_bits
from tests import score_cases as sc

pytestmark = pytest.mark.gpu

TAIL = 16
NAN_BITS, INT_POISON = 0x7FC54321, -77777
FLOATS, INTS = ("logprob", "lse", "zmax", "top_logprob", "top_z"), ("argmax", "top_ids")


@pytest.fixture(scope="module")
def tiny():
    """any context serves the op (it brings its own operands)"""
    from detikzify_amd.model import load
    return load("detikzify-tiny", synthetic=1234)[0]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _poison(name, n):
    if name in INTS:
        return np.full(n + TAIL, INT_POISON, dtype=np.int32)
    return np.full(n + TAIL, NAN_BITS, dtype=np.uint32).view(np.float32)


def operands(c):
    if "_ops" not in c.__dict__:
        c._ops = (f32_to_bits(c.A), f32_to_bits(c.W))
    return c._ops


def call(m, c, k, wt, rows=None, leave=()):
    """one call on the rows `rows` of the case (default: all); `leave` = outputs passed as NULL.  Returns (outputs, kernel record)."""
    Ab, Wb = operands(c)
    rows = np.arange(c.M) if rows is None else np.asarray(rows)
    A = np.ascontiguousarray(Ab[rows])
    tg = np.ascontiguousarray(c.targets[rows])
    M = len(rows)
    names = ("logprob", "lse", "argmax", "zmax") + (("top_ids", "top_logprob", "top_z") if k else ())
    buf = {n: _poison(n, M * (k if n.startswith("top") else 1)) for n in names}
    a = {n: (None if n in leave else _p(buf[n])) for n in names}
    flags = sc.WT if wt else 0
    if k:
        rc = m.lib.dtk_op_score_top(m._ctx, _p(A), _p(Wb), _p(tg), M, c.N, c.K, flags, a["logprob"], a["lse"], a["argmax"], a["zmax"], k,
                                    a["top_ids"], a["top_logprob"], a["top_z"])
    else:
        rc = m.lib.dtk_op_score(m._ctx, _p(A), _p(Wb), _p(tg), M, c.N, c.K, flags, a["logprob"], a["lse"], a["argmax"], a["zmax"])
    m._check(rc, f"{c.name} k={k} wt={wt}")          # (the op's own guard check is part of it)
    code = m.lib.dtk_gemm_last_kernel()
    out = {}
    for n in names:
        size = M * (k if n.startswith("top") else 1)
        own, tail = buf[n][:size], buf[n][size:]
        assert tail.tobytes() == _poison(n, 0).tobytes(), f"{c.name}: {n} written behind its end"
        if n in leave:
            assert own.tobytes() == _poison(n, size)[:size].tobytes(), f"{c.name}: {n} was passed as NULL"
        else:
            out[n] = own.reshape(M, k) if n.startswith("top") else own
    return out, code


def same_bits(a, b, names=None):
    return all(a[n].tobytes() == b[n].tobytes() for n in (names or a))


def device_logits(m, c):
    """the random class: z as dtk_op_gemm stores it for the same operands"""
    Ab, Wb = operands(c)
    z = np.empty((c.M, c.N), dtype=np.uint16)
    m._check(m.lib.dtk_op_gemm(m._ctx, _p(Ab), _p(Wb), None, None, c.M, c.N, c.K, 0, _p(z)), "dtk_op_gemm")
    c.set_logits(bits_to_f32(z))


def _paths():
    out = []
    for cls in sc.CLASSES:
        for path in ("mfma", "g3"):
            if any((sc.family(c.code(0)) == "mfma") == (path == "mfma") for c in sc.cases_of(cls)):
                out.append((cls, path))
    return out


@pytest.mark.parametrize("cls,path", _paths())
def test_score_op_class(tiny, cls, path):
    worst, where, calls, seen = 0.0, None, 0, {}
    for c in sc.cases_of(cls):
        if (sc.family(c.code(0)) == "mfma") != (path == "mfma"):
            continue
        if cls == "random":
            device_logits(tiny, c)
        first = None
        for wt in c.wts:
            for k in c.ks:
                out, code = call(tiny, c, k, wt)
                assert code == c.code(wt), f"{c.name} wt={wt}: kernel record {code:#x}, the routing says {c.code(wt):#x}"
                seen[(c.M, c.N, c.K, wt)] = code
                ok, fig = c.judge(out, k)
                print(f"{c.name} wt={wt} k={k}: |d lse| {fig['d_lse']:.2e}" + ("" if ok else f" {fig}"))
                assert ok, (c.name, wt, k, fig)
                if fig["d_lse"] > worst:
                    worst, where = fig["d_lse"], c.name
                again, _ = call(tiny, c, k, wt)
                assert same_bits(out, again), f"{c.name} wt={wt} k={k}: the second call differs"
                calls += 2
                if first is None:
                    first = out
                # W as fragment-major tiles or not, with or without the top-k kernel behind it: the same bits
                assert same_bits(first, out, ("logprob", "lse", "argmax", "zmax")), f"{c.name} wt={wt} k={k}"
                if k == c.ks[-1] and wt == c.wts[-1]:
                    for m in sorted({0, c.M // 2, c.M - 1}):          # a row as the only row of a call
                        alone, _ = call(tiny, c, k, wt, rows=[m])
                        assert all(alone[n].tobytes() == out[n][m:m + 1].tobytes() for n in out), f"{c.name}: row {m} alone"
                        calls += 1
    rec = ", ".join(f"{M}x{N}x{K} wt={wt}: {code:#x}" for (M, N, K, wt), code in sorted(seen.items())) if path == "g3" else f"{7 | 3 << 4:#x}"
    print(f"{cls} on {path}: {calls} calls, worst |d lse| {worst:.2e} ({where}); kernel records: {rec}")


def test_wide_against_tall_the_same_rows_give_the_same_bits(tiny):
    a, b = sc.pair_cases()
    for wt in (0, 1):
        wide, cw = call(tiny, a, 8, wt)
        tall, ct = call(tiny, b, 8, wt)
        assert sc.family(cw) == "wide" and sc.family(ct) == "tall" and cw == a.code(wt) and ct == b.code(wt)
        assert all(wide[n].tobytes() == tall[n][:a.M].tobytes() for n in wide), wt


def test_outputs_passed_as_null_are_left_alone_and_change_nothing(tiny):
    for c in (next(x for x in sc.cases_of("lit") if x.N == 8200), sc.pair_cases()[0]):
        full, _ = call(tiny, c, 5, 0)
        part, _ = call(tiny, c, 5, 0, leave=("lse", "argmax", "zmax", "top_z"))
        assert set(part) == {"logprob", "top_ids", "top_logprob"} and same_bits(part, {n: full[n] for n in part})
        base, _ = call(tiny, c, 0, 0, leave=("lse", "argmax", "zmax"))
        assert base["logprob"].tobytes() == full["logprob"].tobytes()
