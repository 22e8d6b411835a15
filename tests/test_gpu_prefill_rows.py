"""What sits between the GEMMs of a prefill layer, op by op on the MI355X against the references of tests/prefill_rows_cases.py: RoPE +
Q scatter + KV append (dtk_op_rope_scatter), the norms behind a role (dtk_op_rows_norm), SwiGLU in its three forms (dtk_op_swiglu),
launch_attention in the layouts the product uses (dtk_op_attention_ex) and gather / copy / im2col (dtk_op_rows_move).  Every result
buffer starts as NaN poison and the op's device scratch as 0xFF bytes; what a kernel must not write has to keep its bits, and the op
itself fails if anything behind the end of a result buffer was written.

Besides the bars, the bit identities the code promises: a sliced-K RoPE kernel = the bf16 kernel on bf16(sum of slices); the rows form
with {start + t, start + t} = the start_pos form; launch_rmsnorm_rows_sk on k_sk_reduce's C = its fused Y; k_sk_reduce_swiglu =
k_silu_mul on the bf16 slice sums; the GEMM_SWIGLU epilogue = k_gemm_g3 + k_silu_mul; attention in any layout, batched, grouped = the
contiguous single-problem call with the K / V heads repeated, and a causal tail call = the last rows of the full call; another scratch
poison changes nothing."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from detikzify_amd import _lib
from oracle.ops import f32_to_bits
from tests import prefill_rows_cases as pc

pytestmark = pytest.mark.gpu

ERR_ARG = -1


@pytest.fixture(scope="module")
def tiny():
    """any context serves the ops (they bring their own operands)"""
    from detikzify_amd.model import load
    return load("detikzify-tiny", synthetic=1234)[0]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dtype=None):
    return None if a is None else np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype=dtype))


class Worst:
    def __init__(self):
        self.w = {}

    def add(self, name, fig):
        s, c, a = self.w.get(name, ((0.0, 0.0, 0.0), (0.0, 0.0), (0.0, 0.0)))
        self.w[name] = (tuple(map(max, s, fig["single"])), tuple(map(max, c, fig["chain"])), tuple(map(max, a, fig["attn"])))

    def show(self):
        for name, (s, c, a) in self.w.items():
            print(f"{name}: single-rounding differing {s[0]:.4f} max_ulp {s[1]:.2f} rel_l2 {s[2]:.2e}; chained max_ulp {c[0]:.2f} rel_l2 {c[1]:.2e}; "
                  f"attention max_ulp {a[0]:.2f} rel_l2 {a[1]:.2e}")


def _same(a, b):
    return all(np.array_equal(a[n], b[n]) for n in a)


# ------------------------------------------------------------------------------------------ one call per case type
def call_rope(m, c, fill=0xFF, buf=None, **over):
    buf = buf or c.initial()
    rows = np.stack([c.pos, c.row], axis=1) if c.table else None
    a = dict(form=int(c.S > 0), qkv=c.qkv if c.S == 0 else None, part=c.part.numpy() if c.S else None, S=c.S, part_rows=getattr(c, "part_rows", 0),
             T=c.T, H=c.H, KVH=c.KVH, hd=c.hd, T_max=pc.T_MAX, start=c.start, rows=rows, max_pos=pc.MAX_POS)
    a.update(over)
    qkv, part, rows = _c(a["qkv"]), _c(a["part"], np.float32), _c(a["rows"], np.int32)
    cos, sin = f32_to_bits(c.cos), f32_to_bits(c.sin)
    rc = m.lib.dtk_op_rope_scatter(m._ctx, a["form"], _p(qkv), _p(part), a["S"], a["part_rows"], a["T"], a["H"], a["KVH"], a["hd"], a["T_max"],
                                   a["start"], _p(rows), a["max_pos"], _p(cos), _p(sin), fill, _p(buf["q"]), _p(buf["k"]), _p(buf["v"]))
    return rc, buf


def call_norm(m, c, fill=0xFF, buf=None, **over):
    buf = buf or c.initial()
    if isinstance(c, pc.SkCase):
        a = dict(form=2, X=None, part=c.part.numpy(), S=c.S, part_rows=c.part_rows, w=f32_to_bits(c.w) if c.norm else None, b=None,
                 bias=f32_to_bits(c.bias), res=c.res_buffer(), gate=f32_to_bits(c.gate), flags=c.flags, M=c.M, N=c.N, ldx=0, ldc=c.ldc, ldr=c.ldr, ldy=c.ldy, eps=pc.EPS)
    else:
        a = dict(form=c.form, X=None if c.in_place else c.x_buffer(), part=None, S=0, part_rows=0, w=f32_to_bits(c.w),
                 b=f32_to_bits(c.b) if c.form == 3 else None, bias=None, res=None, gate=None, flags=0, M=c.M, N=c.D, ldx=c.ldx, ldc=0, ldr=0, ldy=c.ldy,
                 eps=pc.LN_EPS if c.form == 3 else pc.EPS)
    a.update(over)
    X, part, res = _c(a["X"]), _c(a["part"], np.float32), _c(a["res"])
    rc = m.lib.dtk_op_rows_norm(m._ctx, a["form"], _p(X), _p(part), a["S"], a["part_rows"], _p(a["w"]), _p(a["b"]), _p(a["bias"]), _p(res), _p(a["gate"]),
                                a["flags"], a["M"], a["N"], a["ldx"], a["ldc"], a["ldr"], a["ldy"], a["eps"], fill, _p(buf.get("c")), _p(buf.get("y")))
    return rc, buf


def call_swiglu(m, c, fill=0xFF, buf=None, **over):
    buf = buf or c.initial()
    a = dict(form=c.form, GU=f32_to_bits(c.GU) if c.form == 0 else None, part=c.part.numpy() if c.form == 1 else None, S=c.S,
             part_rows=getattr(c, "part_rows", 0), A=f32_to_bits(c.A) if c.form == 2 else None, W=f32_to_bits(c.W) if c.form == 2 else None,
             M=c.M, ff=c.ff, K=c.K, ldact=c.ldact)
    a.update(over)
    part = _c(a["part"], np.float32)
    rc = m.lib.dtk_op_swiglu(m._ctx, a["form"], _p(a["GU"]), _p(part), a["S"], a["part_rows"], _p(a["A"]), _p(a["W"]), a["M"], a["ff"], a["K"],
                             a["ldact"], fill, _p(buf["act"]))
    return rc, buf


def call_attn(m, c, fill=0xFF, buf=None, **over):
    buf = buf or c.initial()
    ops = c.operands()
    a = dict(q=ops["q"], k=ops["k"], v=ops["v"], nq=ops["q"].size, nk=ops["k"].size, nv=ops["v"].size, no=buf["o"].size, strides=c.strides(),
             H=c.H, G=c.G, Tq=c.Tq, Tk=c.Tk, hd=c.hd, causal=c.causal, q_offset=c.q_offset, B=c.B)
    a.update(over)
    q, k, v, st = _c(a["q"]), _c(a["k"]), _c(a["v"]), _c(a["strides"], np.int64)
    rc = m.lib.dtk_op_attention_ex(m._ctx, _p(q), a["nq"], _p(k), a["nk"], _p(v), a["nv"], _p(buf["o"]), a["no"], _p(st), a["H"], a["G"], a["Tq"],
                                   a["Tk"], a["hd"], a["causal"], a["q_offset"], a["B"], fill)
    return rc, buf


def call_move(m, c, fill=0xFF, buf=None, **over):
    buf = buf or c.initial()
    a = dict(form=c.form, ids=getattr(c, "ids", None), src={0: getattr(c, "table", None), 1: getattr(c, "src", None), 2: None}[c.form],
             pixels=c.pixels.numpy() if c.form == 2 else None, M=getattr(c, "M", 0), D=c.D, V=getattr(c, "V", 0), lds=getattr(c, "lds", 0),
             ldd={0: c.D, 1: getattr(c, "ldd", 0), 2: c.ldp}[c.form], image=getattr(c, "image", 0), patch=getattr(c, "patch", 0))
    a.update(over)
    ids, src, px = _c(a["ids"], np.int32), _c(a["src"]), _c(a["pixels"], np.float32)
    rc = m.lib.dtk_op_rows_move(m._ctx, a["form"], _p(ids), _p(src), _p(px), a["M"], a["D"], a["V"], a["lds"], a["ldd"], a["image"], a["patch"], fill,
                                _p(buf["dst"]))
    return rc, buf


CALL = {pc.RopeCase: call_rope, pc.NormCase: call_norm, pc.SkCase: call_norm, pc.SwiCase: call_swiglu, pc.AttnCase: call_attn, pc.MoveCase: call_move}


def run(m, c, fill=0xFF, **over):
    rc, buf = CALL[type(c)](m, c, fill, **over)
    m._check(rc, f"{c.name} {sorted(over)}")
    return buf


def judged(m, c, worst, group, fill=0xFF):
    buf = run(m, c, fill)
    ok, fig = c.judge(buf)
    if all(x == x for t in ("single", "chain", "attn") for x in fig[t]):
        worst.add(group, fig)
    assert ok, f"{c.name}: {fig}"
    return buf


@pytest.fixture()
def g3_any_shape(tiny):
    """k_gemm_g3 for shapes of a few blocks (the prefill demands 128); restored afterwards"""
    tiny.set_option("gemm_g3_min_blocks", 1)
    yield tiny
    tiny.set_option("gemm_g3_min_blocks", 128)
    tiny.set_option("gemm_impl", 3)


# ------------------------------------------------------------------------------------------ RoPE, Q scatter, KV append
def test_rope_scatter_against_the_references_and_its_twins(tiny):
    worst = Worst()
    for c in pc.rope_cases():
        buf = judged(tiny, c, worst, "rope " + ("sliced" if c.S else "bf16") + (" rows" if c.table else ""))
        if c.S:         # = the bf16 kernel fed bf16(sum of slices), and another poison between the partial rows changes nothing
            twin = run(tiny, c, form=0, qkv=c.x_bits("f32"), part=None, S=0, part_rows=0)
            assert _same(twin, buf), f"{c.name}: the sliced kernel and the bf16 kernel on the rounded sums differ in bits"
            assert _same(run(tiny, c, fill=0x5A), buf), c.name
        if not c.table:  # = the rows form with {start + t, start + t}
            ident = np.stack([c.pos, c.row], axis=1)
            assert _same(run(tiny, c, rows=ident, start=0), buf), f"{c.name}: the rows form with the identity table differs in bits"
    worst.show()


# ------------------------------------------------------------------------------------------ norms
def test_rows_norms_against_the_references(tiny):
    worst = Worst()
    for c in pc.norm_cases():
        buf = judged(tiny, c, worst, f"norm form {c.form}" + (" GRID" if c.style == "grid" else ""))
        if c.form == 1 or c.in_place:
            assert _same(run(tiny, c, fill=0x5A), buf), c.name
    worst.show()


def test_sk_reduce_against_the_references_and_the_norm_alone(tiny):
    """... and launch_rmsnorm_rows_sk on the C it wrote equals its fused Y bit for bit (same thread -> column map, same order of the sum of
    squares), N = 4100 (the read-back branch) and the misaligned strides included"""
    worst = Worst()
    for c in pc.sk_cases():
        buf = judged(tiny, c, worst, f"sk_reduce{' + norm' if c.norm else ''} {c.style}")
        assert _same(run(tiny, c, fill=0x5A), buf), c.name
        if c.norm:
            y = {"y": np.full((c.M, c.ldy), pc.NAN_Y, dtype=np.uint16)}
            rc, alone = call_norm(tiny, c, buf=y, form=1, X=buf["c"], part=None, S=0, part_rows=0, bias=None, res=None, flags=0, ldx=c.ldc)
            tiny._check(rc, c.name)
            assert np.array_equal(alone["y"], buf["y"]), f"{c.name}: the norm alone and the fused norm differ in bits"
    worst.show()


# ------------------------------------------------------------------------------------------ SwiGLU
def test_silu_mul_against_the_references(tiny):
    worst = Worst()
    for c in pc.swiglu_cases(0):
        judged(tiny, c, worst, "silu_mul" + (" GRID" if c.style == "grid" else "") + (" grid-stride" if pc.silu_grid(c.M, c.ff)[2] else ""))
    worst.show()


def _silu_mul(m, gu_bits, M, ff):
    act = np.full((M, ff), pc.NAN_ACT, dtype=np.uint16)
    gu = _c(gu_bits)
    m._check(m.lib.dtk_op_swiglu(m._ctx, 0, _p(gu), None, 0, 0, None, None, M, ff, 0, ff, 0xFF, _p(act)), "dtk_op_swiglu form 0")
    return act


def test_sk_reduce_swiglu_against_the_references_and_silu_mul(tiny):
    worst = Worst()
    for c in pc.swiglu_cases(1):
        buf = judged(tiny, c, worst, "sk_reduce_swiglu" + (" GRID" if c.style == "grid" else ""))
        assert _same(run(tiny, c, fill=0x5A), buf), c.name
        if c.ff % 8 == 0:        # (k_silu_mul takes whole 16-byte chunks)
            twin = _silu_mul(tiny, f32_to_bits(c.gate_up("f32")), c.M, c.ff)
            assert np.array_equal(twin, buf["act"][:, :c.ff]), f"{c.name}: the reduction and k_silu_mul on the rounded sums differ in bits"
    worst.show()


def test_gemm_swiglu_epilogue_against_the_references_and_the_pair_it_replaces(g3_any_shape):
    m = g3_any_shape
    worst = Worst()
    for c in pc.swiglu_cases(2):
        buf = judged(m, c, worst, f"GEMM_SWIGLU tile {pc.g3_tile(c.M, 2 * c.ff)}")
        assert _same(run(m, c, fill=0x5A), buf), c.name
        # the pair: k_gemm_g3 with the fragment-major W (gemm_impl 4, DTK_GEMM_WT) -> GU, k_silu_mul on it
        m.set_option("gemm_impl", 4)
        gu = np.full((c.M, 2 * c.ff), pc.NAN_Y, dtype=np.uint16)
        A, W = f32_to_bits(c.A), f32_to_bits(c.W)
        m._check(m.lib.dtk_op_gemm(m._ctx, _p(A), _p(W), None, None, c.M, 2 * c.ff, c.K, _lib.DTK_GEMM_WT, _p(gu)), "dtk_op_gemm")
        m.set_option("gemm_impl", 3)
        assert np.array_equal(_silu_mul(m, gu, c.M, c.ff), buf["act"][:, :c.ff]), f"{c.name}: the fused epilogue and GEMM + k_silu_mul differ in bits"
    worst.show()


# ------------------------------------------------------------------------------------------ attention
def _contiguous(m, q, k, v, causal, q_offset):
    """dtk_op_attention: one problem, [H][T][hd], one K / V head per query head"""
    H, Tq, hd = q.shape
    out = np.full((H, Tq, hd), pc.NAN_O, dtype=np.uint16)
    qb, kb, vb = f32_to_bits(q), f32_to_bits(k), f32_to_bits(v)
    m._check(m.lib.dtk_op_attention(m._ctx, _p(qb), _p(kb), _p(vb), H, Tq, k.shape[1], hd, causal, q_offset, _p(out)), "dtk_op_attention")
    return out


@pytest.mark.parametrize("impl", [1, 2])
def test_attention_layouts_against_the_references_and_the_contiguous_call(tiny, impl):
    """every layout, batch and group size against float64, and bit for bit against dtk_op_attention on each batch's problem laid out
    contiguously with K / V head h // G repeated (so: any layout = contiguous, batch b of nbatch = b alone, GQA = MHA on repeated heads);
    the last r rows as a tail call (Tq = r, q_offset = Tk - r) equal those rows of the full causal call"""
    tiny.set_option("attn_impl", impl)
    worst = Worst()
    try:
        for c in pc.attn_cases():
            buf = judged(tiny, c, worst, f"attention impl {impl} {c.layout}")
            got = buf["o"][c._index("o", c.B, c.H, c.Tq)]                 # [B][H][Tq][hd]
            heads = [h // c.G for h in range(c.H)]
            for b in range(c.B):
                q, k, v = c.q[b % c.q.shape[0]], c.k[b % c.k.shape[0]][heads], c.v[b % c.v.shape[0]][heads]
                plain = _contiguous(tiny, q, k, v, c.causal, c.q_offset)
                assert np.array_equal(plain, got[b]), f"{c.name} batch {b}: the layout and the contiguous call differ in bits"
                if c.causal and c.Tq > 1:
                    r = min(3, c.Tq - 1)
                    tail = _contiguous(tiny, q[:, c.Tq - r:], k, v, 1, c.Tk - r)
                    assert np.array_equal(tail, got[b][:, c.Tq - r:]), f"{c.name} batch {b}: a tail call of {r} rows differs in bits"
            assert _same(run(tiny, c, fill=0x5A), buf), c.name
    finally:
        tiny.set_option("attn_impl", 0)
    worst.show()


# ------------------------------------------------------------------------------------------ gather, copy, im2col
def test_rows_move_is_bit_exact(tiny):
    worst = Worst()
    for c in pc.move_cases():
        buf = judged(tiny, c, worst, "rows_move")
        assert _same(run(tiny, c, fill=0x5A), buf), c.name
    worst.show()


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_touch_nothing(tiny, g3_any_shape):
    """everything the prefill would never hand these kernels: DTK_ERR_ARG, nothing launched, every buffer as it was — and the same call
    without the fault is taken"""
    R = lambda **kw: pc._case(pc.RopeCase, 64, 4, 2, **kw)
    rope, rope_rows, rope_sk = R(start=3), R(table="a"), R(start=3, S=3)
    rms, rms_sk, ln = pc._case(pc.NormCase, 0, 5, 72), pc._case(pc.NormCase, 1, 5, 4), pc._case(pc.NormCase, 3, 5, 1152)
    sk = pc._case(pc.SkCase, 3, 260, 1, pc.DTK_EPI_BIAS | pc.DTK_EPI_RESIDUAL, 0)
    silu, skswi, g3 = pc._case(pc.SwiCase, 0, 5, 24), pc._case(pc.SwiCase, 1, 3, 24, S=3), pc._case(pc.SwiCase, 2, 100, 80, K=136)
    att = pc._case(pc.AttnCase, "prefill", 64, 4, 2, 17, 64, 1, causal=1, q_offset=47)
    vit = pc._case(pc.AttnCase, "vit", 72, 2, 1, 17, 17, 1)
    gather, copy, im = (pc._case(pc.MoveCase, 0, D=8), pc._case(pc.MoveCase, 1, D=8), pc._case(pc.MoveCase, 2, ldp=592))
    far_pos, far_row = np.array([[3, 8], [4, 9], [pc.MAX_POS, 10], [3, 11], [4, 12]]), np.array([[3, 8], [4, 9], [5, pc.T_MAX], [3, 11], [4, 12]])
    st = att.strides()
    odd, wide_k, k_sh_off = st.copy(), st.copy(), st.copy()
    odd[1] += 1                    # q_st: odd
    wide_k[4] += 8                 # k_st: the last key row of the last head ends behind the buffer
    k_sh_off[3] += 4               # k_sh % 8 != 0: the MFMA kernel's 16-byte loads (refused under attn_impl 2 only)
    bad = [(rope, dict(hd=96)), (rope, dict(hd=32)), (rope, dict(KVH=3)), (rope, dict(start=pc.T_MAX - 4)), (rope, dict(max_pos=7)),
           (rope_rows, dict(rows=far_pos)), (rope_rows, dict(rows=far_row)), (rope_sk, dict(S=0)), (rope_sk, dict(S=9)), (rope_sk, dict(part_rows=4)),
           (rms, dict(N=68)), (ln, dict(N=1148)), (rms_sk, dict(N=6)), (rms, dict(ldx=64)), (sk, dict(N=258)), (sk, dict(S=9)), (sk, dict(S=0)),
           (sk, dict(bias=None)), (sk, dict(res=None)), (sk, dict(ldc=256)), (sk, dict(flags=13, gate=None)), (sk, dict(flags=9)), (sk, dict(flags=2)),
           (silu, dict(ff=20)), (silu, dict(ldact=32)), (skswi, dict(S=9)), (skswi, dict(S=0)), (skswi, dict(ff=22)), (skswi, dict(ldact=20)),
           (g3, dict(K=120)), (g3, dict(K=132)), (g3, dict(ff=72)), (g3, dict(ldact=82)),
           (att, dict(strides=odd)), (att, dict(strides=wide_k)), (att, dict(nk=att.size["k"] - 3 * 64 - 8)), (att, dict(no=att.size["o"] - 16)),       # (behind the last row a cache has 3 spare rows, O 8 spare columns) (att, dict(G=3)),
           (att, dict(hd=48)), (vit, dict(nv=vit.size["v"] - 8)),
           (gather, dict(ids=np.array([0, 6, 3, 7, 0, 6, 5]))), (gather, dict(ids=np.array([0, 6, 3, -1, 0, 6, 5]))), (gather, dict(D=12)),
           (copy, dict(lds=4)), (copy, dict(D=12)), (im, dict(ldd=584))]
    for c, over in bad:
        rc, buf = CALL[type(c)](tiny, c, **over)
        init = c.initial()
        assert rc == ERR_ARG, (c.name, over.keys(), rc)
        assert _same(buf, init), (c.name, list(over))
    # the launcher's own refusal (fewer blocks than "gemm_g3_min_blocks" asks for), and the MFMA kernel's operands under attn_impl 2
    tiny.set_option("gemm_g3_min_blocks", 128)
    rc, buf = call_swiglu(tiny, g3)
    assert rc == ERR_ARG and _same(buf, g3.initial())
    tiny.set_option("gemm_g3_min_blocks", 1)
    tiny.set_option("attn_impl", 2)
    try:
        rc, buf = call_attn(tiny, att, strides=k_sh_off, nk=att.size["k"] + 16, k=np.concatenate([att.operands()["k"], np.zeros(16, dtype=np.uint16)]))
        assert rc == ERR_ARG and _same(buf, att.initial())
        rc, buf = call_attn(tiny, att, hd=32, Tk=1, Tq=1)
        assert rc == ERR_ARG and _same(buf, att.initial())
    finally:
        tiny.set_option("attn_impl", 0)
    # (and the same calls without the fault are taken)
    for c in (rope, rope_rows, rope_sk, rms, rms_sk, ln, sk, silu, skswi, g3, att, vit, gather, copy, im):
        ok, fig = c.judge(run(tiny, c))
        assert ok, (c.name, fig)
