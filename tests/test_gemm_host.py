"""The host side of the prefill GEMM op tests (no GPU): every buffer tests/test_gpu_gemm.py hands dtk_op_gemm_ex is built here too; the
poison is complete; the grid classes have the properties their bit-equality rests on; the coverage the case lists claim is computed from
the mirrored routing of tests/gemm_cases.py; the float32 oracle chain, judged like a device result, passes every case; the distance of
the two references over the random chained outputs is what the case file records and the GPU bar is taken from; each deliberately
wrong reference misses the bar at every case it applies to; the C ABI's additions."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from oracle.ops import bits_to_f32
from tests import gemm_cases as gc

ROOT = Path(__file__).resolve().parent.parent
FAMILIES = tuple(dict.fromkeys(gc.ONE_CHAIN_FAMILIES + gc.SLICED_FAMILIES))


def _runs():
    for fam in FAMILIES:
        for v in gc.variants(fam):
            for c in gc.cases_of(fam):
                yield c, v


def test_cases_are_named_uniquely_and_the_poison_is_complete():
    names = set()
    for c in gc.all_cases():
        assert c.name not in names, c.name
        names.add(c.name)
        init, idx = c.initial(), c.cells()
        assert init.size == c.c_off + c.M * c.ldc and len(np.unique(idx)) == c.M * c.N and idx.max() < init.size      # M rows exactly
        mask = np.ones(init.size, dtype=bool)
        mask[idx] = False
        assert (init[mask] == gc.NAN_C).all(), c.name
        assert c.inplace or (init == gc.NAN_C).all()
        a, w = c.a_buffer().reshape(c.M, c.lda), c.w_buffer().reshape(c.N, c.ldw)
        assert a.shape[1] % 8 == 0 and w.shape[1] % 8 == 0 and c.K % 8 == 0
        assert (a[:, c.K:] == gc.NAN_GAP).all() and (w[:, c.K:] == gc.NAN_GAP).all()
        if c.tag not in ("patch-embed", "vit-inplace", "image-query", "pool-head"):
            assert c.lda == c.K + 8 and c.ldw == c.K + 24
        b = c.bias_buffer()
        assert (b[:c.b_off] == gc.NAN_GAP).all() and b.size == c.b_off + c.N
        r = c.res_buffer()
        assert (r[:c.r_off] == gc.NAN_GAP).all() and (r[c.r_off:].reshape(c.M, c.ldr)[:, c.N:] == gc.NAN_GAP).all() and r.size == c.r_off + c.M * c.ldr
        assert c.inplace or not (c.flags & gc.RES) or c.ldr != c.ldc or c.tag == "vit-inplace"
    assert np.isnan(bits_to_f32(np.array([gc.NAN_C, gc.NAN_GAP], dtype=np.uint16)).numpy()).all() and gc.NAN_C != gc.NAN_GAP


def test_grid_operands_have_one_value_per_output():
    """the two conditions of the grid class: every fp32 partial sum is an integer below 2^24 whatever the order, and the gate's sigmoid
    is far from a rounding boundary; the GELU grid: every pre-activation's GELU is, none left out, and the Linear's rounding shows"""
    s = gc.sigmoid64(gc.GATE_GRID)
    assert float(gc.boundary_distance(s)) >= gc.MARGIN
    assert float(gc.boundary_distance(torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -16, 1.0 - 2.0 ** -9 - 2.0 ** -17, 3.0]).double())[0]) < 2.0 ** -7      # (the measure itself)
    for c in gc.all_cases():
        if c.cls == "grid":
            A, W = c.A[~torch.isnan(c.A).any(1)], c.W[~torch.isnan(c.W).any(1)]
            assert float(A.abs().max()) <= 4 and float(W.abs().max()) <= 4 and bool((A == A.round()).all()) and bool((W == W.round()).all())
            assert 16 * c.K < 2 ** 24
            assert bool(((c.bias * 8) == (c.bias * 8).round()).all()) and float(c.bias.abs().max()) <= 4
            res = c.res[torch.isfinite(c.res)]
            assert bool(((res * 8) == (res * 8).round()).all())
            assert (c.A != 0).float().mean() > 0.8 and (c.W != 0).float().mean() > 0.8              # dense
        elif c.cls == "gelu":
            kind = "erf" if c.flags & gc.ERF else "tanh"
            pre = c.accumulate() + c.bias.double()
            assert float(pre.abs().max()) <= 4 and bool((c.A.sum(1) == 1).all()) and c.hot[0] == c.K - 1
            assert float(gc.gelu_distance(gc.r64(pre), kind).min()) >= gc.MARGIN              # every output, none excluded
            assert bool((gc.r64(pre) != pre).any())
            a, b = c.reference(), c.reference(mutate="linear_unrounded")
            assert int((a != b).sum()) >= 1, c.name
        elif c.cls == "order":
            for k0, k1 in gc.slice_ranges(c.K, c.S):
                part = (c.A[:, k0:k1].double().abs() @ c.W[:, k0:k1].double().abs().t())
                assert float(part.max()) <= 2.0 ** 28 and bool((part.float().double() == part).all())
            assert bool((c.reference() == 4 * (c.S // 3) * torch.outer(c.A[:, c.K // c.S].clamp(max=2), c.W[:, c.K // c.S].clamp(-2, 2))).all())
            assert bool((c.reference(mutate="one_chain") == 0).all())
    for kind in ("erf", "tanh"):
        assert all(len(a) >= 20 for a in gc.gelu_allowed(kind))


def test_the_axes_of_the_issue_are_all_there():
    one, sk = gc.one_chain_cases(), gc.sliced_cases()
    assert {c.K for c in one} >= {8, 40, 64, 72, 128, 136, 192, 200, 256, 328, 4304}
    assert {c.M for c in one} >= {1, 31, 32, 33, 63, 65, 127, 129, 255, 257}
    assert {c.N for c in one} >= {1, 7, 30, 36, 31, 33, 63, 65, 127, 129, 255, 257, 264, 520, 1032, 2056}
    assert all(c.K == 136 and c.M <= 257 for c in one if c.N >= 264)
    assert {c.ldc - c.N for c in one} >= {0, 8, 4, 2} and {c.ldr - c.N for c in one if not c.inplace} >= {0, 8, 4, 2}
    for off in ("c_off", "r_off", "b_off"):
        assert {getattr(c, off) for c in one} >= {0, 4, 2, 1}, off
    for cls, epis in (("grid", {"none", "bias", "bias_res", "inplace", "gated", "res"}), ("gelu", {"erf", "tanh"}),
                      ("random", {"none", "bias", "erf", "tanh", "bias_res", "inplace", "gated", "res"})):
        assert {c.epi for c in one if c.cls == cls} >= epis, cls
    assert {c.contain for c in one} >= {"a_nan", "w_nan", "res_inf"}
    pe = next(c for c in one if c.tag == "patch-embed")
    assert pe.K == pe.lda == pe.ldw == 592 and pe.ldr != pe.ldc
    assert any(c.tag == "vit-inplace" and c.inplace for c in one) and any(c.M == 1 for c in one if c.tag == "image-query")
    assert {(c.K, c.S) for c in sk if c.cls == "grid"} == {(K, S) for K in (128, 200, 576, 4304) for S in range(1, 9)}
    lens = {tuple((k1 - k0) // 64 for k0, k1 in gc.slice_ranges(c.K, c.S)) for c in sk}
    assert any(0 in l for l in lens) and any(1 in l and max(l) > 1 for l in lens) and (2, 2, 2, 2, 1) in lens       # empty, one tile long, ragged
    assert any(c.inplace for c in sk) and {c.ldc - c.N for c in sk} >= {0, 8, 4, 2} and all(c.N % 4 == 0 for c in sk)
    assert max(c.M * c.N * c.K for c in gc.all_cases() if c.K != 4304) <= 300 * 2100 * 600
    big = [c for c in gc.all_cases() if c.M > 257 or c.N > 2056 or (c.K > 600 and c.K != 4304 and c.cls != "order")]
    assert sorted((c.M, c.N, c.K) for c in big) == [(384, 2056, 128), (512, 1032, 128)] and all(c.tag == "xcd" and c.S for c in big)     # k_gemm_g3<SL>'s orientation needs them
    assert gc.anchor(gc.one_chain_cases()[0]).name == "mfma-t1-D3" and gc.anchor(sk[0]).name == "sk-tall-rm-lds"


def test_the_mirrored_routing_reaches_every_instantiation_path_and_fallback():
    seen, paths, br, xcd = set(), set(), set(), set()
    for c, v in _runs():
        code = gc.route(c, v)
        seen.add(gc.strip(code))
        fam, tile = code & 15, (code >> 4) & 15
        paths.add((fam, (code >> 14) & 3))
        br |= gc.branches(c, v)
        bm, bn = {1: (64, 64), 2: (128, 64), 3: (128, 128), 4: (64, 32), 5: (32, 32), 6: (256, 128), 7: (128, 256), 0: (4, 64)}[tile]
        if fam in (1, 2, 3, 5) and (c.N + bn - 1) // bn > 8 and (c.M + bm - 1) // bm > 1:
            xcd.add((fam, tile))                # the second group of the XCD map with more than one row block
    missing = gc.instantiations() - seen
    assert not missing, sorted(hex(m) for m in missing)
    assert paths >= {(3, 1), (3, 2), (4, 1), (4, 2), (5, 1), (5, 2), (1, 0), (2, 0), (6, 0)}
    assert br >= {"tiles", "lds", "lds_bias16", "lds_bias_scalar", "lds_rvec", "lds_rscalar", "direct_forced", "direct_n8", "direct_ldc8", "vec", "novec",
                  "nvec", "scalar_cols", "rvec", "rscalar", "bvec", "bscalar", "sk_lds", "sk_direct", "red_vec", "red_novec", "red_rvec", "red_rscalar",
                  "red_bvec", "red_bscalar"}, br
    assert xcd >= {(1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (2, 3), (3, 6), (3, 7), (5, 6), (5, 7)}, xcd
    # the fall-through is on show: a k_gemm_g3 variant below K = 128 and a k_gemm_glds variant below K = 64 end at k_gemm_mfma
    g3 = gc.variants("g3-tall")[0]
    assert {gc.route(c, g3) & 15 for c in gc.one_chain_cases()} == {1, 3} and {gc.route(c, gc.variants("glds")[0]) & 15 for c in gc.one_chain_cases()} == {1, 2}
    # the k_gemm_g3 ring: nk = 2, 3, 4 and 6 > every stage count, with and without a tail
    nk = {(c.K // 64, c.K % 64 != 0) for c in gc.one_chain_cases() if c.K >= 128}
    assert nk >= {(2, False), (2, True), (3, False), (3, True), (4, False), (5, True)}


def test_reference_against_the_float32_oracle_and_the_bar_it_sets():
    wu = wr = 0.0
    where = None
    for c in gc.all_cases():
        ok, fig = c.judge(c.place(c.ref("f32")))
        assert ok, (c.name, fig)
        if c.kind != "chain":
            continue
        for d in [c] + [c.redraw(s) for s in range(1, gc.REDRAWS + 1)]:
            u, r = d.reference_distance()
            if u > wu or r > wr:
                where = d.name
            wu, wr = max(wu, u), max(wr, r)
    print(f"float64 vs float32 reference, random chained outputs and {gc.REDRAWS} redraws each: worst {wu:.2f} ulps, rel-L2 {wr:.2e} (last raised by {where})")
    assert 0.5 * gc.MEASURED_CHAIN_ULPS <= wu <= 1.25 * gc.MEASURED_CHAIN_ULPS, wu
    assert 0.5 * gc.MEASURED_CHAIN_RL2 <= wr <= 1.25 * gc.MEASURED_CHAIN_RL2, wr
    assert gc.CHAIN_ULPS == min(4.01, 2 * gc.MEASURED_CHAIN_ULPS) and gc.CHAIN_RL2 == min(2e-3, 2 * gc.MEASURED_CHAIN_RL2)
    assert (gc.SINGLE_RL2, gc.SINGLE_ULPS, gc.SINGLE_FRAC) == (1e-3, 2.01, 0.05)


@pytest.mark.parametrize("mutation", gc.MUTATIONS)
def test_a_wrong_reference_misses_the_bar(mutation):
    """each deliberately wrong reference, judged as a device result, fails in every case it applies to — and applies to at least one"""
    hit = 0
    for c in gc.all_cases():
        if not c.applies(mutation):
            continue
        ok, fig = c.judge(c.wrong(mutation))
        assert not ok, (mutation, c.name, fig)
        hit += 1
    assert hit > 0
    assert len(gc.MUTATIONS) == len(set(gc.MUTATIONS)) == 15


def test_header_declares_the_entry_and_symbols_list_it():
    header = (ROOT / "include" / "dtk.h").read_text()
    table = (ROOT / "INTEGRATION.md").read_text()
    for name in ("dtk_op_gemm_ex", "dtk_gemm_last_kernel"):
        assert re.search(rf"^int\s+{name}\(", header, re.M), name
        assert name in _lib.SYMBOLS and name in table, name
    decl = re.search(r"^int\s+dtk_op_gemm_ex\((.*?)\);", header, re.M | re.S).group(1)
    assert len(_lib.SYMBOLS["dtk_op_gemm_ex"][1]) == decl.count(",") + 1 == 25
    assert re.search(r"#define\s+DTK_ABI_VERSION\s+7\b", header) and _lib.DTK_ABI_VERSION == 7          # an additive entry: the ABI number stays
    for macro, value in (("DTK_EPI_GELU_ERF", gc.ERF), ("DTK_EPI_GELU_TANH", gc.TANH), ("DTK_GEMM_INPLACE", gc.INPLACE), ("DTK_EPI_GATED_RESIDUAL", gc.GATED),
                         ("DTK_GEMM_NAIVE", gc.NAIVE), ("DTK_GEMM_WT", gc.WT), ("DTK_GEMM_SL", gc.SL), ("DTK_GEMM_KSLICES_SHIFT", gc.KS_SHIFT)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", header), macro
        assert getattr(_lib, macro) == value
    assert '"gemm_g3_tile"' in header and "gemm_g3_tile" in table and '"gemm_g3_tile"' in (ROOT / "detikzify_amd" / "csrc" / "dtk_api.hip").read_text()
    kh = (ROOT / "detikzify_amd" / "csrc" / "kernels.h").read_text()
    assert "GEMM_KCODE" in kh and re.search(r"^int gemm_last_kernel\(\);", kh, re.M)
