"""The host side of the multi-vector decode GEMV op tests (no GPU): every input tests/test_gpu_gemv_mv.py feeds to k_gemv_mv is built
here too; the coverage the case lists claim is computed from the mirrored table of launch_mv_nb (shape -> U, waves, persistent, blocks
per CU, with the fp8 rule), not taken on trust; the float64 reference against the float32 chain on oracle.ops.linear (their worst
distance sets the bar of the chained outputs); each deliberately wrong reference misses the bar at every case it applies to; the C
ABI's addition."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

from detikzify_amd import _lib
from tests import gemv_cases as gc
from tests import gemv_mv_cases as mc

ROOT = Path(__file__).resolve().parent.parent
NEW = ("dtk_op_gemv_mv_role",)
ROLE_ID = lambda r: f"{gc.PRO_NAME[r[0]]}-{gc.EPI_NAME[r[1]]}-{r[2]}"


def _everything():
    return mc.all_cases() + [c for c, _, _ in mc.persistent_cases()]


def test_cases_exist_and_are_named_uniquely():
    names = set()
    for c in _everything():
        assert c.name not in names, c.name
        names.add(c.name)
        assert len(set(c.pos)) == c.nb and 0 not in c.pos and gc.T_MAX - 1 in c.pos and max(c.pos) < gc.T_MAX
        for s in c.slots[1:]:           # one W, norm_w, wscale; x (and the residual) per slot
            assert s.W is c.W and s.norm_w is c.norm_w and s.wscale is c.wscale and not np.array_equal(s.x.numpy(), c.slots[0].x.numpy())
            assert c.epi != gc.RESID or c.N < 8 or not np.array_equal(s.res.numpy(), c.slots[0].res.numpy())
        for name, b in c.initial().items():
            poison = np.isnan(gc.bits_to_f32(b).numpy()) if b.dtype == np.uint16 else np.isnan(b)
            assert poison.all() or (c.epi == gc.RESID and name == "y"), (c.name, name)
        if c.fmt == "fp8":
            e = np.log2(c.wscale.numpy())
            assert (e == np.round(e)).all() and (e.max() - e.min() >= 6 or c.N < 7)
        if c.x_layout:                  # the fragment-order input: slot b's values where the kernel reads them, poison everywhere else
            x = c.x_buffer()
            assert x.size == (c.K + 31) // 32 * 512
            for b in range(c.nb):
                cks = np.arange(c.K // 8)
                assert np.array_equal(x.reshape(-1, 8)[(cks >> 2) * 64 + (cks & 3) * 16 + b].reshape(-1), c.x_rows()[b])      # k_gemv_mv's own index
            assert int((x != mc.NAN_X).sum()) <= c.nb * c.K
    for role in mc.ROLES:
        pro, epi, fmt = role
        for nb in mc.NBS:
            cs = mc.role_cases(*role, nb)
            assert set(mc.K_OF[fmt]) <= {c.K for c in cs} and any(c.grid for c in cs), (role, nb)
            assert {(c.active, c.bs_null) for c in cs} == set(mc.ACTIVE[nb]), (role, nb)
            if epi == gc.SWIGLU:
                assert {8, 24, 88} <= {c.ff for c in cs} and all(c.ff % 32 for c in cs)
            elif epi == gc.QKV:
                assert set(gc.HEADS) <= {(c.H, c.KVH) for c in cs}
            else:
                assert {1, 37, 130, 257} <= {c.N for c in cs}
            if pro == gc.COPY:
                assert {0, 1} == {c.x_layout for c in cs}
    # the active sets of the issue
    assert {a for a, _ in mc.ACTIVE[2]} == {(1, 1), (1, 0), (0, 1)} and {a for a, _ in mc.ACTIVE[4]} == {(1, 1, 1, 1), (1, 0, 1, 1), (0, 1, 1, 0), (0, 0, 0, 1)}
    assert all(any(null and all(a) for a, null in mc.ACTIVE[nb]) for nb in mc.NBS)
    big = {c.K: c for c in mc.role_cases(gc.COPY, gc.RESID, "bf16", 4)}
    assert {8192, 8200, 11008, 14336} <= set(big) and all(big[K].N <= 130 and big[K].N * K * 2 < 4e6 for K in (8192, 8200, 11008, 14336))


@pytest.mark.parametrize("role", mc.ROLES, ids=ROLE_ID)
def test_every_instantiation_meets_the_paths_the_case_list_claims(role):
    """from (U, waves) of every (nb, shape) and the K the role's cases have: 1, 2 and >= 3 k-groups (both parities of the two-stage loop),
    a group wholly inside the row and a ragged one, under PRO_RMSNORM both norm paths, a unit tail wherever the role's unit granularity
    (QKV 64 per head, SWIGLU 8, else 1) leaves one possible; for (COPY, RESID) at nb 4 the dynamic-LDS attribute with and without the
    forced shape, up to the largest request of a product model"""
    pro, epi, fmt = role
    seen = {}
    for nb in mc.NBS:
        cases = mc.role_cases(*role, nb)
        ks = sorted({c.K for c in cases})
        for shape in mc.SHAPES:
            U, waves, persistent, bpc = mc.shape_of(pro, epi, fmt, nb, shape)
            assert persistent == (bpc > 0) and (fmt != "fp8" or waves <= 8)
            # the K that reach this instantiation: above 64 KiB of x every shape runs as shape 3
            mine = [K for K in ks if mc.launched_shape(shape, epi, nb, K, 0) == shape]
            g = {gc.groups(fmt, K, U)[0] for K in mine}
            assert 1 in g and 2 in g and max(g) >= 3, (role, nb, shape, sorted(g))
            assert any(gc.has_full_group(fmt, K, U) for K in mine) and any(gc.has_ragged_group(fmt, K, U) for K in mine), (role, nb, shape)
            if pro == gc.RMSNORM:
                assert any(K // 8 <= 512 for K in mine) and any(K // 8 > 512 for K in mine), (role, nb, shape, "norm paths")
                assert {4096, 4104 if fmt == "bf16" else 4112} <= set(mine)
            gran = {gc.QKV: 64, gc.SWIGLU: 8}.get(epi, 1)
            if gran % waves:
                assert any(c.units % waves for c in cases), (role, nb, shape, "no unit tail")
            seen[(nb, shape)] = (U, waves, persistent, bpc, sorted(g))
    if (pro, epi) == (gc.COPY, gc.RESID):
        assert {seen[(nb, s)][0] for nb in mc.NBS for s in (0, 1, 2)} == ({8, 4} if fmt == "bf16" else {4, 2})      # UR: 8 at nb 1, 4 above
        ks = sorted({c.K for c in mc.role_cases(*role, 4)})
        waves3 = mc.shape_of(pro, epi, fmt, 4, 3)[1]
        raised = [K for K in ks if mc.lds_bytes(4, K, waves3) > 64 * 1024]
        assert 8192 in raised and mc.launched_shape(0, epi, 4, 8192, 0) == 0                  # the attribute in a shape of the caller's choice
        assert all(mc.launched_shape(s, epi, 4, K, 0) == 3 for K in raised if K > 8192 for s in (-1, 0, 1, 2, 3))
        assert max(raised) == 14336 and mc.lds_bytes(4, 14336, 16) == 112 * 1024 + 4 * 16 * 4 + 64 <= mc.LDS_CU
    for key, v in sorted(seen.items()):
        print(f"{ROLE_ID(role)} nb {key[0]} shape {key[1]}: U {v[0]}, {v[1]} waves, persistent {v[2]} ({v[3]} blocks per CU), k-groups {v[4]}")


def test_the_mirrored_table_is_launch_mv_nbs():
    """shape_of() against the MV(...) lines of launch_mv_nb themselves and the fp8 rule of the MV macro"""
    src = (ROOT / "detikzify_amd" / "csrc" / "kernels_decode_mv.hip").read_text()
    body = src[src.index("static void launch_mv_nb("):src.index("#undef MV")]
    rows = re.findall(r"(default|case (\d)): MV\(PRO_(\w+), EPI_(\w+), NB, (\d), (\w+), (\d+), (true|false), (\d)\);", body)
    assert len(rows) == 16
    pro_of, epi_of = {"RMSNORM": gc.RMSNORM, "COPY": gc.COPY}, {"QKV": gc.QKV, "SWIGLU": gc.SWIGLU, "LOGITS": gc.LOGITS, "RESID": gc.RESID}
    assert "constexpr int UR = NB == 1 ? 8 : 4;" in body
    for _, shape, pro, epi, R, U, waves, persistent, bpc in rows:
        for nb in mc.NBS:
            u = (8 if nb == 1 else 4) if U == "UR" else int(U)
            assert R == "1" and mc.shape_of(pro_of[pro], epi_of[epi], "bf16", nb, int(shape or 0)) == (u, int(waves), persistent == "true", int(bpc)), (pro, epi, shape, nb)
    assert "if (pro == PRO_RMSNORM) MV(PRO_RMSNORM, EPI_STORE, NB, 1, 2, 4, false, 0);" in body and "MV(PRO_COPY, EPI_STORE, NB, 1, 2, 4, false, 0);" in body
    assert "launch_mv_t<PRO, EPI, NBV, R, ((U) >= 2 ? (U) / 2 : 1), ((W) == 16 ? 8 : (W)), P, true>(a, s, BPC)" in src
    assert mc.shape_of(gc.COPY, gc.RESID, "fp8", 1, 3) == (2, 8, True, 1) and mc.shape_of(gc.RMSNORM, gc.QKV, "fp8", 4, 1) == (1, 8, True, 2)
    assert "const int lds = (int)((size_t)NB * (a.K >> 3) * 16 + (size_t)NB * WAVES * 4 + 64);" in src and mc.lds_bytes(4, 8192, 16) == 65536 + 256 + 64


def test_default_shape_mirror():
    for nb, K, d, epi, want in ((1, 4096, 4096, gc.QKV, 0), (2, 4096, 4096, gc.RESID, 0), (2, 11008, 4096, gc.RESID, 3), (2, 4096, 4096, gc.QKV, 0),
                                (4, 4096, 4096, gc.QKV, 1), (4, 4096, 4096, gc.RESID, 3), (4, 4096, 4096, gc.LOGITS, 3), (4, 11008, 4096, gc.RESID, 3),
                                (2, 32776, 0, gc.LOGITS, 3)):
        assert mc.default_shape(epi, nb, K, d) == want, (nb, K, d, epi)
    assert mc.launched_shape(1, gc.RESID, 4, 8200, 0) == 3 and mc.launched_shape(1, gc.RESID, 4, 8192, 0) == 1


def test_persistent_cases_take_a_second_trip_for_some_waves_only():
    cases = mc.persistent_cases()
    assert {(c.pro, c.epi, c.fmt, s) for c, _, s in cases} == {(p, e, f, s) for f in ("bf16", "fp8") for p, e in mc.PERSISTENT_ROLES for s in (1, 2, 3)}
    for c, first, shape in cases:
        U, waves, persistent, bpc = mc.shape_of(c.pro, c.epi, c.fmt, 4, shape)
        assert persistent and c.K == 64 and c.nb == 4 and first == mc.NOMINAL_CUS * bpc * waves and first < c.units < 2 * first
        assert not all(c.active) and sum(c.active) >= 2


def test_reference_against_the_float32_oracle_and_the_bar_it_sets():
    """the float32 chain run through the buffers and judged like a device result passes everywhere; the worst distance of the chained
    outputs is what tests/gemv_mv_cases.py records, and the GPU bar is twice it under the caps"""
    wu = wr = 0.0
    for c in _everything():
        ok, fig = c.judge(c.written(c.outs("f32")))
        assert ok, (c.name, fig)
        for d in [c] + mc.redraws(c):
            u, r = d.reference_distance()
            wu, wr = max(wu, u), max(wr, r)
    print(f"float64 vs float32 reference, chained outputs: worst {wu:.2f} ulps, rel-L2 {wr:.2e}")
    # (the float32 matmul's summation order belongs to the BLAS at hand: the recorded figures may move a little, not by a factor)
    assert 0.5 * mc.MEASURED_CHAIN_ULPS <= wu <= 1.25 * mc.MEASURED_CHAIN_ULPS, wu
    assert 0.5 * mc.MEASURED_CHAIN_RL2 <= wr <= 1.25 * mc.MEASURED_CHAIN_RL2, wr
    assert mc.CHAIN_ULPS == min(4.01, 2 * mc.MEASURED_CHAIN_ULPS) and mc.CHAIN_RL2 == min(2e-3, 2 * mc.MEASURED_CHAIN_RL2)
    assert (mc.SINGLE_RL2, mc.SINGLE_ULPS, mc.SINGLE_FRAC) == (1e-3, 2.01, 0.05)


@pytest.mark.parametrize("mutation", mc.MUTATIONS)
def test_a_wrong_reference_misses_the_bar(mutation):
    """slot b computed from slot b ^ 1's x; every slot from slot 0's x; the RoPE angle and cache row of the next active slot; every slot's
    K / V in slot 0's cache; an idle slot written; the (8-k piece, slot) indices of the fragment order swapped on the input and on the
    SwiGLU output; the residual of the next slot; and gemv_cases' per-slot faults on every live slot — judged as a device result in every
    case they apply to"""
    hit = 0
    for c in _everything():
        if not c.applies(mutation):
            continue
        ok, fig = c.judge(c.written(c.outs(mutate=mutation), mutation))
        assert not ok, (mutation, c.name, fig)
        hit += 1
    assert hit > 0


def test_header_declares_the_function_and_symbols_list_it():
    header = (ROOT / "include" / "dtk.h").read_text()
    for name in NEW:
        assert re.search(rf"^int\s+{name}\(", header, re.M), name
        assert name in _lib.SYMBOLS, name
        decl = re.search(rf"^int\s+{name}\((.*?)\);", header, re.M | re.S).group(1)
        assert len(_lib.SYMBOLS[name][1]) == decl.count(",") + 1, name
    assert len(_lib.SYMBOLS["dtk_op_gemv_mv_role"][1]) == 30
    assert len(_lib.SYMBOLS["dtk_op_gemv_mv"][1]) == 10           # (the earlier entry stays)
    assert re.search(r"#define\s+DTK_ABI_VERSION\s+7\b", header) and _lib.DTK_ABI_VERSION == 7
    table = (ROOT / "INTEGRATION.md").read_text()
    assert all(f"`{name}(" in table for name in NEW)
    src = (ROOT / "detikzify_amd" / "csrc" / "dtk_ops.hip").read_text()
    body = src[src.index("int dtk_op_gemv_mv_role("):]
    body = body[:body.index("\n}\n")]
    assert "MvShapeScope scope(epi, shape);" in body and "set_gemv_mv_shape(epi, -1)" in src          # the shape is restored on every exit path
    assert body.index("r.upload(s)") > max(body.index(m) for m in ("DTK_ERR_ARG, \"%s: %d vectors", "x_layout == 1 && pro == PRO_RMSNORM", "bs_null && !active[b]"))
    kern = (ROOT / "detikzify_amd" / "csrc" / "kernels_decode_mv.hip").read_text()
    assert "tests/test_gpu_parity_mv.py::test_multi_vector_gemv_is_the_single_sequence_gemv_per_vector" in kern and "tests/test_gpu_gemv_mv.py" in kern
