"""The host side of the single-sequence decode GEMV op tests (no GPU): every input tests/test_gpu_gemv.py feeds to k_gemv is built here
too; the coverage the case lists claim is computed from the mirrored (R, U, waves, persistent, KS) tables, not taken on trust; the
float64 reference against the float32 chain on oracle.ops.linear (their worst distance sets the bar of the chained outputs); each
deliberately wrong reference misses the bar at every case it applies to; the C ABI's addition."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

from detikzify_amd import _lib
from tests import gemv_cases as gc

ROOT = Path(__file__).resolve().parent.parent
NEW = ("dtk_op_gemv_role",)


def test_cases_exist_and_are_named_uniquely():
    names = set()
    for c in gc.all_cases():
        assert c.name not in names, c.name
        names.add(c.name)
        assert c.pos in (gc.T_MAX - 1, gc.POS_IN) and c.pos != 0
        for name, b in c.initial().items():
            poison = np.isnan(gc.bits_to_f32(b).numpy()) if b.dtype == np.uint16 else np.isnan(b)
            assert poison.all() or (c.epi == gc.RESID and name == "y"), (c.name, name)
        if c.fmt == "fp8":
            e = np.log2(c.wscale.numpy())
            assert (e == np.round(e)).all() and (e.max() - e.min() >= 6 or c.N < 7)
        if c.pro == gc.ATTN:
            assert c.K == c.H * c.hd and bool((c.pl >= 0).all()) and bool((c.pl.sum(1) > 0).all())
            if c.S >= 3:
                assert bool((c.pm[:, c.S - 2] == -1e30).all()) and bool((c.pl[:, c.S - 2] == 0).all()) and bool((c.po[:, c.S - 2] == 0).all())
    assert set(gc.ROLES) == set(gc.TABLE)
    by = lambda pro, epi, fmt: [c for c in gc.role_cases(pro, epi, fmt)]
    for fmt in ("bf16", "fp8", "mxfp4"):
        ks = {8, 72, 520, 1032, 2048, 2056, 4096, 4104, 8200, 11008} if fmt != "fp8" else {2048, 4096, 11008, 4112, 8208}
        for pro, epi in ((gc.COPY, gc.RESID), (gc.RMSNORM, gc.LOGITS), (gc.COPY, gc.STORE), (gc.RMSNORM, gc.STORE), (gc.RMSNORM, gc.SWIGLU)):
            if (pro, epi, fmt) not in gc.TABLE:
                continue
            cs = by(pro, epi, fmt)
            assert ks <= {c.K for c in cs}, (pro, epi, fmt)
            assert any(c.grid for c in cs)
            if epi == gc.SWIGLU:
                assert {8, 24, 88} <= {c.ff for c in cs}
            else:
                assert {1, 37, 130, 257} <= {c.N for c in cs}
        cs = by(gc.RMSNORM, gc.QKV, fmt)
        assert {(h, kvh, hd) for hd in (128, 64) for h, kvh in gc.HEADS} <= {(c.H, c.KVH, c.hd) for c in cs if not c.grid}
        assert {c.pos for c in cs} == {gc.T_MAX - 1, gc.POS_IN}
        cs = by(gc.ATTN, gc.RESID, fmt)
        assert {1, 3, 4, 5, 16} <= {c.S for c in cs} and {(2, 128), (4, 128), (4, 64), (8, 64)} <= {(c.H, c.hd) for c in cs}
        assert {37, 256} <= {c.N for c in cs} and any(c.S % 4 for c in cs)
    # the persistent shapes: every instantiation the issue lists, a second trip for some waves only (at the nominal CU count)
    shapes = gc.persistent_shapes()
    assert {(gc.RMSNORM, gc.QKV, "bf16", v) for v in (3, 4, 5)} | {(gc.RMSNORM, gc.SWIGLU, "bf16", v) for v in (3, 4, 5)} | \
        {(gc.COPY, gc.RESID, "bf16", 4), (gc.COPY, gc.RESID, "bf16", 5), (gc.RMSNORM, gc.LOGITS, "bf16", 1),
         (gc.RMSNORM, gc.QKV, "mxfp4", -1), (gc.RMSNORM, gc.SWIGLU, "mxfp4", -1)} | \
        {(p, e, "fp8", v) for p, e in ((gc.RMSNORM, gc.QKV), (gc.RMSNORM, gc.SWIGLU), (gc.COPY, gc.RESID)) for v in (6, 7, 8, 9)} == set(shapes)
    for pro, epi, fmt, v in shapes[:3] + shapes[-3:]:
        case, first = gc.persistent_case(pro, epi, fmt, v, 64, gc.NOMINAL_CUS)
        assert case.K == 64 and first < case.units < 2 * first      # (some waves take a second chunk, the others do not)


@pytest.mark.parametrize("role", gc.ROLES, ids=lambda r: f"{gc.PRO_NAME[r[0]]}-{gc.EPI_NAME[r[1]]}-{r[2]}")
def test_every_instantiation_meets_the_paths_the_case_list_claims(role):
    """from (U, waves, KS) and the K the role's cases have: 1, 2 and >= 3 k-groups (both parities of the two-stage loop), a group wholly
    inside the row and a ragged one, for split-K a wave without a group and waves with unequal counts, for PRO_RMSNORM both norm paths,
    and a unit tail wherever the role's unit granularity (QKV 32 per head at least, SWIGLU 8, else 1) leaves one possible"""
    pro, epi, fmt = role
    cases = gc.role_cases(*role)
    ks = sorted({c.K for c in cases})
    for v, (R, U, waves, bpc, KS) in gc.TABLE[role].items():
        g0 = {gc.groups(fmt, K, U, KS)[0] for K in ks}
        assert 1 in g0 and 2 in g0 and max(g0) >= 3, (role, v, sorted(g0))
        assert any(gc.has_full_group(fmt, K, U) for K in ks) and any(gc.has_ragged_group(fmt, K, U) for K in ks), (role, v)
        if KS > 1:
            per = [gc.groups(fmt, K, U, KS) for K in ks]
            assert any(0 in p for p in per), (role, v, "no idle split-K wave")
            assert any(min(p) >= 1 and max(p) > min(p) for p in per), (role, v, "no unequal counts among busy waves")
        if pro == gc.RMSNORM:
            assert any(K // 8 <= 128 * waves for K in ks) and any(K // 8 > 128 * waves for K in ks), (role, v, "norm paths")
        per_block = R * (waves // KS)
        gran = {gc.QKV: 32, gc.SWIGLU: 8}.get(epi, 1)
        if gran % per_block:
            assert any(c.units % per_block for c in cases), (role, v, "no unit tail")


def test_reference_against_the_float32_oracle_and_the_bar_it_sets():
    """the float32 chain run through the buffers and judged like a device result passes everywhere; the worst distance of the chained
    outputs is what tests/gemv_cases.py records, and the GPU bar is twice it under the caps"""
    wu = wr = 0.0
    cases = gc.all_cases() + [gc.persistent_case(*s, hd, gc.NOMINAL_CUS)[0] for s in gc.persistent_shapes() for hd in ((128, 64) if s[1] == gc.QKV else (128,))]
    for c in cases:
        ok, fig = c.judge(c.written(c.reference("f32")))
        assert ok, (c.name, fig)
        for d in [c] + gc.redraws(c):
            u, r = d.reference_distance()
            wu, wr = max(wu, u), max(wr, r)
    print(f"float64 vs float32 reference, chained outputs: worst {wu:.2f} ulps, rel-L2 {wr:.2e}")
    # (the float32 matmul's summation order belongs to the BLAS at hand: the recorded figures may move a little, not by a factor)
    assert 0.5 * gc.MEASURED_CHAIN_ULPS <= wu <= 1.25 * gc.MEASURED_CHAIN_ULPS, wu
    assert 0.5 * gc.MEASURED_CHAIN_RL2 <= wr <= 1.25 * gc.MEASURED_CHAIN_RL2, wr
    assert gc.CHAIN_ULPS == min(4.01, 2 * gc.MEASURED_CHAIN_ULPS) and gc.CHAIN_RL2 == min(2e-3, 2 * gc.MEASURED_CHAIN_RL2)
    assert (gc.SINGLE_RL2, gc.SINGLE_ULPS, gc.SINGLE_FRAC) == (1e-3, 2.01, 0.05)


@pytest.mark.parametrize("mutation", gc.MUTATIONS)
def test_a_wrong_reference_misses_the_bar(mutation):
    """pos off by one; the RoPE partner's sign flipped; the fp8 scale of row r0 on its partner r0 + hd/2; gate and up swapped; the last
    k head taken for a v head; one wave-load of K dropped / counted twice; the last 16-byte chunk of x dropped; the scale of row
    r + 1 / r - 1; res + p rounded once (GRID cases: on random operands that is at most one ulp); the last split left out of the
    combine; the combine not divided by L; block c's scale on block c + 1 — judged as a device result in every case it applies to"""
    hit = 0
    for c in gc.all_cases():
        if not c.applies(mutation):
            continue
        ok, fig = c.judge(c.written(c.reference(mutate=mutation)))
        assert not ok, (mutation, c.name, fig)
        hit += 1
    assert hit > 0


def test_default_variant_table_names_rows_of_the_table():
    for pro, epi, fmt in gc.ROLES:
        for d in (0, 2048, 4096):
            for K in (2048, 4096, 11008):
                v = gc.default_variant(pro, epi, fmt, K, d)
                assert v in gc.TABLE[(pro, epi, fmt)] or (v == 0 and fmt == "bf16"), (pro, epi, fmt, d, K, v)
    reached = {gc.default_variant(gc.COPY, gc.RESID, "bf16", K, d) for d in (2048, 4096) for K in (2048, 4096, 11008)}
    assert reached == {1, 15, 10}
    assert {gc.default_variant(gc.ATTN, gc.RESID, "bf16", d, d) for d in (2048, 4096)} == {1, 8}
    assert gc.default_variant(gc.RMSNORM, gc.SWIGLU, "bf16", 2048, 2048) == 5 and gc.default_variant(gc.RMSNORM, gc.LOGITS, "bf16", 4096, 4096) == 3


def test_header_declares_the_function_and_symbols_list_it():
    header = (ROOT / "include" / "dtk.h").read_text()
    for name in NEW:
        assert re.search(rf"^int\s+{name}\(", header, re.M), name
        assert name in _lib.SYMBOLS, name
        decl = re.search(rf"^int\s+{name}\((.*?)\);", header, re.M | re.S).group(1)
        assert len(_lib.SYMBOLS[name][1]) == decl.count(",") + 1, name
    assert len(_lib.SYMBOLS["dtk_op_gemv_role"][1]) == 33
    assert re.search(r"#define\s+DTK_ABI_VERSION\s+7\b", header) and _lib.DTK_ABI_VERSION == 7
    table = (ROOT / "INTEGRATION.md").read_text()
    assert all(name in table for name in NEW)
    src = (ROOT / "detikzify_amd" / "csrc" / "kernels_decode.hip").read_text()
    assert "launch_gemv_f8_variant(pro, epi, f8_variant(), a, s)" in src          # the process default goes through the explicit-variant twin
