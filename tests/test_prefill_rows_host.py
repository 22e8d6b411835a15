"""The host side of the prefill row-kernel and attention-layout op tests (no GPU): every input tests/test_gpu_prefill_rows.py feeds to
the kernels is built here too; the coverage the case lists claim is computed from the mirrored thread-to-column maps of
tests/prefill_rows_cases.py, not taken on trust; the float32 oracle chain, judged like a device result, passes every case; the worst
distance of the two references over the chained outputs is what the case file records and the GPU bar is taken from; each deliberately
wrong reference misses the bar at every case it applies to; the C ABI's additions."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from oracle.ops import bits_to_f32
from tests import prefill_rows_cases as pc

ROOT = Path(__file__).resolve().parent.parent
NEW = ("dtk_op_rope_scatter", "dtk_op_rows_norm", "dtk_op_swiglu", "dtk_op_attention_ex", "dtk_op_rows_move")


def test_cases_are_named_uniquely_and_the_poison_is_complete():
    names, payloads = set(), {}
    for c in pc.all_cases():
        assert c.name not in names, c.name
        names.add(c.name)
        for name, b in c.initial().items():
            if isinstance(c, pc.NormCase) and c.in_place:
                continue                        # (Y == X: the buffer is the input)
            assert b.dtype == np.uint16 and np.isnan(bits_to_f32(b).numpy()).all(), (c.name, name)
            assert len(np.unique(b)) == 1
            payloads.setdefault((c.group, name), set()).add(int(b.reshape(-1)[0]))
        assert set(c.kinds()) == set(c.initial()), c.name
        mask = c.write_mask()
        assert all(m.any() for m in mask.values()), c.name
    assert all(len(v) == 1 for v in payloads.values())
    for group in pc.GROUPS:                     # within a call every result buffer has a payload of its own
        own = [next(iter(v)) for (g, _), v in payloads.items() if g == group]
        assert len(own) == len(set(own)), group
    assert pc.NAN_IN not in {p for v in payloads.values() for p in v} and pc.NAN_GAP not in {p for v in payloads.values() for p in v}


def test_rope_cases_reach_every_instantiation_and_edge():
    cs = pc.rope_cases()
    assert {(c.hd, c.H, c.KVH, c.start) for c in cs if c.S == 0 and not c.table} == {(hd, h, k, s) for hd in (128, 64) for h, k in pc.HEADS for s in (3, 11)}
    for rows in (False, True):          # k_sk_rope_scatter<S, HD> and k_sk_rope_scatter_rows<S, HD>: 16 instantiations each
        assert {(c.S, c.hd) for c in cs if c.S and bool(c.table) == rows} == {(S, hd) for S in range(1, 9) for hd in (128, 64)}
        assert {c.hd for c in cs if c.S == 0 and bool(c.table) == rows} == {128, 64}
    for c in cs:
        assert c.T == 5 and int(c.pos.min()) > 0 and int(c.row.max()) < pc.T_MAX and int(c.pos.max()) + 1 < pc.MAX_POS
        if c.table:
            assert (c.pos != c.row).all() and (np.diff(c.pos) < 0).any()          # the positions restart mid-table
        else:
            assert c.start in (3, 11)
        if c.S == 0:
            v = c.reference()["v"]
            assert (v == 0x8000).any() and (v == pc.NAN_IN).any()                   # -0.0 and the NaN payload arrive as bits
        else:
            assert c.part_rows > c.T and np.isnan(c.part[:, c.T:].numpy()).all()
            mags = [float(c.part[s, :c.T].abs().mean()) for s in range(c.S)]
            assert c.S == 1 or max(mags) / min(mags) >= 3
    assert any(int(c.row.max()) == pc.T_MAX - 1 for c in cs if not c.table) and any(int(c.row.max()) == pc.T_MAX - 1 for c in cs if c.table)
    # how often the float64 chain differs from the float32 chain (the double rounding of the add)
    diff = tot = 0
    for c in cs:
        a, b = c.place(c.reference("f32")), c.place(c.reference())
        for n in ("q", "k", "v"):
            diff += int((a[n] != b[n]).sum())
            tot += int(c.write_mask()[n].sum())
        assert c.S or np.array_equal(a["v"], b["v"])
    print(f"RoPE outputs where the float64 chain differs from the float32 chain: {diff} of {tot}")
    assert diff <= 1e-3 * tot


def test_norm_cases_reach_every_path():
    cs = pc.norm_cases()
    f0 = [c for c in cs if c.form == 0]
    assert {c.D for c in f0} == set(pc.RMS_D) and {c.M for c in f0} == {1, 5}
    assert {pc.rows_per_block_tail(c.M) for c in f0} == {1}                      # M = 1 and M = 5: a lone row in the last 4-row block
    trips = {max(pc.rms_lane_trips(c.D)) for c in f0} | {min(pc.rms_lane_trips(c.D)) for c in f0}
    assert {0, 1, 2} <= trips and max(trips) >= 4
    assert any(0 in pc.rms_lane_trips(c.D) and 1 in pc.rms_lane_trips(c.D) for c in f0)       # (some lanes idle beside busy ones)
    assert any(len(set(pc.rms_lane_trips(c.D))) == 2 and max(pc.rms_lane_trips(c.D)) == 2 for c in f0)
    f1 = [c for c in cs if c.form == 1]
    assert {c.D for c in f1} == set(pc.SK_ROWS_N) and {c.M for c in f1} == {1, 5}
    assert {pc.sk_thread_trips(c.D)[0] for c in f1} == {1, 2}
    for f in (f0, f1):
        assert all(c.ldx > c.D for c in f) and any(c.ldy > c.D for c in f) and any(c.ldy == c.D for c in f)
        assert any(c.style == "grid" for c in f) and any(c.has_tiny for c in f)
        for c in f:
            if c.has_tiny:
                assert float(c.x[c.M // 2].abs().max()) < 2.0 ** -7
    f3 = [c for c in cs if c.form == 3]
    assert {(c.D, c.M, c.in_place, c.ldx) for c in f3} == {(72, 6, True, 72), (1152, 5, False, 1160)}
    assert max(pc.rms_lane_trips(72)) == 1 and sum(pc.rms_lane_trips(72)) == 9


def test_sk_reduce_cases_reach_every_path():
    cs = pc.sk_cases()
    for norm in (0, 1):
        sub = [c for c in cs if c.norm == norm and c.style != "grid" and c.flags in pc.SK_FLAGS]
        assert {c.S for c in sub} == set(range(1, 9)) and {c.N for c in sub} == set(pc.SK_N)
        assert {(c.flags, c.mis) for c in sub} == {(f, m) for f in pc.SK_FLAGS for m in (0, 1)}
    assert {pc.sk_reduce_grid_y(c.N, c.norm) for c in cs if not c.norm} == {1, 2, 3}
    assert all(pc.sk_reduce_grid_y(c.N, c.norm) == 1 for c in cs if c.norm)
    fused = [c for c in cs if c.norm]
    for branch in ("keep", "readback"):
        sub = [c for c in fused if pc.sk_norm_branch(c.N) == branch]
        assert {pc.sk_vector_paths(c) for c in sub} >= {(True, True, True), (False, False, False)}, branch
        assert {c.flags for c in sub} >= set(pc.SK_FLAGS)
    assert {pc.sk_thread_trips(c.N)[0] for c in fused} >= {1, 2, 3}
    assert any(pc.sk_thread_trips(c.N) == (2, 1) for c in fused)                  # N = 4100: thread 0 alone takes a second trip
    assert any(c.style == "grid" for c in cs) and any(c.style == "exact" for c in cs) and any(c.flags & pc.DTK_EPI_GATED_RESIDUAL for c in cs)
    for c in cs:
        assert c.part_rows > c.M and np.isnan(c.part[:, c.M:].numpy()).all() and c.N % 4 == 0
        if c.style == "exact":             # every fp32 sum of the slices is exact: C has ONE rounding
            assert bool((pc.slice_sum(c.part[:, :c.M], c.S, "f32").double() == pc.slice_sum(c.part[:, :c.M], c.S, "f64")).all())


def test_swiglu_cases_reach_every_path():
    f0, f1, f2 = (pc.swiglu_cases(f) for f in (0, 1, 2))
    assert {(c.ff, c.M) for c in f0 if c.style == "random"} == {(ff, M) for ff in pc.SILU_FF for M in (1, 5)} | {(8200, 1030)}
    loops = [c for c in f0 if pc.silu_grid(c.M, c.ff)[2]]
    assert [(c.M, c.ff) for c in loops] == [pc.SILU_BIG] and pc.silu_grid(*pc.SILU_BIG)[:2] == (4096, 1055750)
    assert 1030 * 8200 * 2 * 3 + 3 * 512 <= 64 << 20                                   # GU + ACT fit the 64 MiB op scratch
    for c in f0:
        if c.style == "random":
            g = c.GU[:, :c.ff]
            assert c.ff < 80 or (float(g.min()) < -15 and float(g.max()) > 15)
    assert {(c.S, c.ff) for c in f1 if c.style == "random"} >= {(S, ff) for S in range(1, 9) for ff in (pc.SKSWI_FF[S % 4], pc.SKSWI_FF[(S + 2) % 4])}
    assert {c.ff for c in f1} >= set(pc.SKSWI_FF) and {c.S for c in f1 if c.style == "random"} == set(range(1, 9))
    assert {pc.sk_swiglu_grid_y(c.ff) for c in f1} == {1, 2} and all(c.ldact == c.ff + 4 for c in f1)
    assert {c.K for c in f2} == set(pc.G3_K) and {c.ff for c in f2} == set(pc.G3_FF) and {c.M for c in f2} == set(pc.G3_M)
    assert {pc.g3_k_tiles(c.K) for c in f2} == {(2, False), (3, True), (4, True), (9, False)}
    tiles = {}
    for c in f2:
        tiles.setdefault(pc.g3_tile(c.M, 2 * c.ff), []).append(c)
        assert c.ff % 16 == 0 and c.K >= 128
    assert set(tiles) == {(256, 128), (128, 256)}                                   # both orientations occur ...
    for t, sub in tiles.items():
        assert any(pc.g3_part_filled_block(c.M, c.ff) for c in sub), t            # ... each with a part-filled pair-ordered column block
        assert any(c.ff > t[1] // 2 or not pc.g3_part_filled_block(c.M, c.ff) for c in sub), t      # ... and with a full one
    for c in f2:                          # the issue's rule: the wide tile for M <= 128 with 128 < 2 ff <= 256
        if c.M <= 128 and 128 < 2 * c.ff <= 256:
            assert pc.g3_tile(c.M, 2 * c.ff) == (128, 256), c.name
    assert any(c.style == "grid" for c in f0) and any(c.style == "grid" for c in f1)


def test_attention_cases_reach_every_layout_and_edge():
    cs = pc.attn_cases()
    by = lambda l: [c for c in cs if c.layout == l]
    pre = by("prefill")
    assert {c.hd for c in pre} == {128, 64} and {c.G for c in pre} == {1, 2, 4} and {c.B for c in pre} == {1, 3}
    assert {c.Tq for c in pre} >= {1, 17, 65} and {c.Tk for c in pre} >= {1, 5, 64, 65, 130}
    assert all(c.causal and c.q_offset == c.Tk - c.Tq for c in pre)
    for hd in (128, 64):
        sub = [c for c in pre if c.hd == hd]
        # (Tq = Tk = 65 itself: its first block needs one key tile and its second holds one query, so no wave skips a loaded tile; that
        # happens where q_offset > 0 puts a block's early waves a whole tile before its last query, as in 65 x 130)
        assert any(c.Tq == c.Tk == 65 for c in sub) and any(pc.attn_wholly_masked_tiles(c) for c in sub)
        assert {c.G for c in sub} == {1, 2, 4} and {pc.attn_key_tiles(c) for c in sub} >= {1, 2, 3}
    for c in pre:
        st = dict(zip(("q_sh", "q_st", "q_sb", "k_sh", "k_st", "k_sb", "v_sh", "v_st", "v_sb", "o_sh", "o_st", "o_sb"), c.strides()))
        assert st["k_sh"] > c.Tk * c.hd and st["o_sh"] == c.hd and st["o_st"] > c.H * c.hd and st["q_sh"] == c.Tq * c.hd
        ops = c.operands()
        assert (ops["k"] == pc.NAN_GAP).sum() == c.B * c.KVH * 3 * c.hd           # rows >= Tk of every head hold NaN
    assert all(c.hd == 72 and not c.causal for l in ("vit", "cross", "pool") for c in by(l))
    assert {c.B for c in by("vit")} == {1, 3} and all(c.strides()[1] == 3 * c.H * c.hd for c in by("vit"))
    assert all(c.Tk == 5 and c.strides()[5] == 0 and c.strides()[8] == 0 for c in by("cross")) and {c.B for c in by("cross")} == {1, 3}
    assert all(c.Tq == 1 and c.strides()[2] == 0 and c.strides()[4] == 2 * c.H * c.hd for c in by("pool")) and {c.Tk for c in by("pool")} >= {1, 5, 64, 65, 130}
    for c in cs:                          # every stride pattern stays inside its buffer, and the result cells are disjoint
        ops, st = c.operands(), c.strides()
        for i, n in enumerate("qkv"):
            nh, nt = (c.H, c.Tq) if n == "q" else (c.KVH, c.Tk)
            assert (c.B - 1) * st[3 * i + 2] + (nh - 1) * st[3 * i] + (nt - 1) * st[3 * i + 1] + c.hd <= ops[n].size == c.size[n], (c.name, n)
        assert int(c.write_mask()["o"].sum()) == c.B * c.H * c.Tq * c.hd


def test_move_cases():
    cs = pc.move_cases()
    g = [c for c in cs if c.form == 0]
    assert {c.D for c in g} == {8, 2056} and all({0, c.V - 1} <= set(c.ids.tolist()) and len(set(c.ids.tolist())) < len(c.ids) for c in g)
    assert {c.D for c in cs if c.form == 1} == {8, 2056} and all(c.lds != c.ldd for c in cs if c.form == 1)
    assert 2056 // 8 == 257                  # 257 chunks: thread 0 of the 256 takes a second trip
    im = [c for c in cs if c.form == 2]
    assert {c.ldp for c in im} == {592, 600} and all(c.image == 28 and c.patch == 14 for c in im)
    for c in im:
        px = c.pixels.double()
        lo, hi = px.to(torch.bfloat16).double(), None
        assert bool((lo != px).float().mean() > 0.7)
        ulp = torch.exp2(torch.floor(torch.log2(px.abs())) - 7)
        assert bool((((px - lo).abs() / ulp) == 0.5).any())                         # ties


def test_reference_against_the_float32_oracle_and_the_bar_it_sets():
    """the float32 chain run through the buffers and judged like a device result passes everywhere; the worst distance of the chained
    outputs is what tests/prefill_rows_cases.py records, and the GPU bar is twice it under the caps"""
    wu = wr = 0.0
    where = None
    for c in pc.all_cases():
        ok, fig = c.judge(c.place(c.reference("f32")))
        assert ok, (c.name, fig)
        for d in [c] + pc.redraws(c):
            u, r = d.reference_distance()
            if u > wu or r > wr:
                where = d.name
            wu, wr = max(wu, u), max(wr, r)
    print(f"float64 vs float32 reference, chained outputs of the cases and their redraws: worst {wu:.2f} ulps, rel-L2 {wr:.2e} (last raised by {where})")
    tu, tr = pc.short_row_distance()
    print(f"... and over {pc.SHORT_ROWS} redraws of the shortest rows (D = 4, 8): worst {tu:.2f} ulps, rel-L2 {tr:.2e}")
    wu, wr = max(wu, tu), max(wr, tr)
    assert 0.5 * pc.MEASURED_CHAIN_ULPS <= wu <= 1.25 * pc.MEASURED_CHAIN_ULPS, wu
    assert 0.5 * pc.MEASURED_CHAIN_RL2 <= wr <= 1.25 * pc.MEASURED_CHAIN_RL2, wr
    assert pc.CHAIN_ULPS == min(4.01, 2 * pc.MEASURED_CHAIN_ULPS) and pc.CHAIN_RL2 == min(2e-3, 2 * pc.MEASURED_CHAIN_RL2)
    assert (pc.SINGLE_RL2, pc.SINGLE_ULPS, pc.SINGLE_FRAC) == (1e-3, 2.01, 0.05) and (pc.ATTN_RL2, pc.ATTN_ULPS) == (2e-3, 4.01)


@pytest.mark.parametrize("mutation", pc.MUTATIONS)
def test_a_wrong_reference_misses_the_bar(mutation):
    """each deliberately wrong reference, judged as a device result, fails in every case it applies to — and applies to at least one"""
    hit = 0
    for c in pc.all_cases():
        if not c.applies(mutation):
            continue
        ok, fig = c.judge(c.place(c.reference(mutate=mutation)))
        assert not ok, (mutation, c.name, fig)
        hit += 1
    assert hit > 0
    assert len(pc.MUTATIONS) == len(set(pc.MUTATIONS)) == 23


def test_header_declares_the_functions_and_symbols_list_them():
    header = (ROOT / "include" / "dtk.h").read_text()
    table = (ROOT / "INTEGRATION.md").read_text()
    for name in NEW:
        assert re.search(rf"^int\s+{name}\(", header, re.M), name
        assert name in _lib.SYMBOLS, name
        decl = re.search(rf"^int\s+{name}\((.*?)\);", header, re.M | re.S).group(1)
        assert len(_lib.SYMBOLS[name][1]) == decl.count(",") + 1, name
        assert name in table, name
    assert re.search(r"#define\s+DTK_ABI_VERSION\s+7\b", header) and _lib.DTK_ABI_VERSION == 7
    assert re.search(r"#define\s+DTK_EPI_GATED_RESIDUAL\s+8\b", header) and pc.DTK_EPI_GATED_RESIDUAL == 8
    kh = (ROOT / "detikzify_amd" / "csrc" / "kernels.h").read_text()
    assert re.search(r"^bool attention_mfma_operands\(const AttnArgs& a\);", kh, re.M)
