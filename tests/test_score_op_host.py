"""The host side of the scoring-head op tests (no GPU): the cases of tests/score_cases.py are sharp.  The unmutated float32 chain, judged
like a device result, passes every case and its distance from the float64 reference is what the case file records; every mutant is
rejected; the coverage the case list claims is computed from the mirrored maps; the logits of every non-random class are exact in fp32
in two k orders; the routing record is documented where the launchers' other records are."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import score_cases as sc

ROOT = Path(__file__).resolve().parent.parent


def _by_size():
    return sorted(sc.all_cases(), key=lambda c: c.M * c.N)


def test_cases_are_named_uniquely_and_hold_the_shapes_of_the_issue():
    cs = sc.all_cases()
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    shapes = {(c.M, c.N, c.K) for c in cs}
    assert shapes >= set(sc.MFMA_SHAPES) | set(sc.G3_SHAPES) | set(sc.PAIR)
    assert max(c.M for c in cs) <= 300 and max(c.N for c in cs) <= 16512 and max(c.K for c in cs) <= 256
    assert {c.N for c in sc.cases_of("flat")} == set(sc.FLAT_N)
    assert {c.cls for c in cs} == set(sc.CLASSES)
    for c in cs:
        assert c.K % 8 == 0 and c.K >= 8 and c.targets.min() >= 0 and c.targets.max() < c.N and c.targets.dtype == np.int32, c.name
        assert c.ks == tuple(k for k in (0, 1, 5, 8) if k <= c.N)
    one = next(c for c in cs if (c.M, c.N, c.K) == (1, 8, 8) and c.cls == "lit")
    assert 8 in one.ks                                                     # M = 1, k = N = 8
    # the routing of the issue's shapes: which of them take k_gemm_g3, tall or wide; each g3 case runs with W's fragment-major copy too
    fam = lambda M, N, K: sc.family(sc.route(M, N, K, 0))
    assert all(fam(*s) == "mfma" for s in sc.MFMA_SHAPES)
    assert [fam(*s) for s in sc.G3_SHAPES] == ["wide", "tall", "tall", "tall"] and [fam(*s) for s in sc.PAIR] == ["wide", "tall"]
    assert fam(300, 16512, 256) == "wide" and fam(300, 16512, 256) != sc.family(sc.route(300, 16512, 256, 0, cus=304))       # (the rounds depend on the CU count)
    assert sc.route(70, 16257, 128, 1) == 7 | 7 << 4 | 1 << 13 and sc.route(257, 16257, 136, 0) == 7 | 6 << 4 and sc.route(130, 8200, 64, 1) == 7 | 3 << 4
    assert sc.family(sc.route(70, 16256, 128, 0)) == "mfma" and sc.family(sc.route(70, 16257, 120, 0)) == "mfma"              # the two thresholds
    assert all(c.wts == ((0,) if sc.family(c.code(0)) == "mfma" else (0, 1)) for c in cs)
    # NT classes
    nts = {c.NT for c in cs}
    assert {1, 2, 64, 65} <= nts and max(nts) >= 128
    assert any(c.N % 128 == 1 and c.NT > 1 for c in cs) and any(c.N % 128 == 0 and c.NT > 1 for c in cs)
    # k > NT, all k best in one tile, the k best in k different tiles
    assert any(c.NT < 5 and 8 in c.ks for c in cs)
    tiles = lambda c: [len(set((c.ref()["top_ids"][m] >> 7).tolist())) for m in range(c.M)]
    small = [c for c in sc.cases_of("ties") if c.N <= 8200]
    assert any(1 in tiles(c) for c in small) and any(8 in tiles(c) for c in small)
    # the pair's shared rows are the same rows on the same lm_head
    a, b = sc.pair_cases()
    assert torch.equal(a.W, b.W) and torch.equal(a.A, b.A[:a.M]) and np.array_equal(a.targets, b.targets[:a.M])


def test_logits_are_exact_in_fp32_in_two_k_orders():
    """ascending and reversed 32-chunks, one fp32 accumulator: the float64 dot's bits, and (channel classes) a bf16 number already"""
    for c in sc.all_cases():
        if not c.exact:
            continue
        want = c.dot64()
        for order in (range(0, c.K, 32), reversed(range(0, c.K, 32))):
            acc = torch.zeros(c.M, c.N)
            for k0 in order:
                acc = acc + c.A[:, k0:k0 + 32] @ c.W[:, k0:k0 + 32].t()
            assert torch.equal(acc.double(), want), c.name
        z = c.z64()
        if c.cls != "grid":
            assert torch.equal(z, want), c.name                           # no two distinct values collide after rb
            assert float(z.max()) <= 8 and float(z.min()) >= -1016
        else:
            assert float(c.A.abs().max()) <= 4 and float((c.W * 64).abs().max()) <= 4 and bool(((c.W * 64) == (c.W * 64).round()).all())
            assert 16 * c.K < 2 ** 24 and (c.K < 128 or bool((z != want).any()))      # a real rounding
        assert float(z.max()) <= 8


def test_class_properties():
    for c in sc.all_cases():
        z = c.z64().numpy()
        r = c.ref()
        if c.cls == "lit":
            hi = np.array(sc.LO)[c.base] + sc.LIT
            assert np.array_equal(z.max(1), hi) and set(np.unique(z)) <= {-24.0, -12.0, -4.0, 8.0}, c.name
            h = (z == hi[:, None]).sum(1)
            want = hi + np.log(h + (c.N - h) * np.exp(-sc.LIT))
            assert np.abs(r["lse"] - want).max() < 1e-9 and h.max() <= 247
            assert h.max() == 1 or np.log(h.max() / (h.max() - 1)) > 200 * sc.LSE_BAR
        elif c.cls == "flat":
            assert np.abs(r["lse"] - (z[:, 0] + np.log(c.N))).max() < 1e-12 and (z == z[:, :1]).all() and 1 / c.N > 40 * sc.LSE_BAR
        elif c.cls == "spread":
            tm = np.stack([z[:, t * 128:(t + 1) * 128].max(1) for t in range(c.NT)], 1)
            assert (tm % 4 == 0).all() and ((tm == tm.max(1, keepdims=True)).sum(1) == 1).all() and tm.max() == 8      # one tile holds the maximum
            assert z.min() <= -1000 or c.NT < 14
            if c.NT >= 14:                                                 # far tiles fold to exactly 0 in fp32, near ones do not
                w = np.exp((tm - tm.max(1, keepdims=True)).astype(np.float32))
                assert (w == 0).sum(1).min() >= c.NT - 27 and ((w > 0) & (w < 1)).sum(1).min() >= 1
            assert {int(t) for t in tm.argmax(1)} == {0, c.NT // 2, c.NT - 1}
        elif c.cls == "ties":
            for k in c.ks[1:]:                                             # the k-th and the (k + 1)-th entry are equal in every row
                assert ((z >= r["top_z"][:, k - 1:k]).sum(1) >= min(k + 1, c.N)).all(), (c.name, k)
            kinds = set()
            for s in sc.tie_sets(c.N)[:c.K - 2]:
                a, b = s[0], s[1]
                same_half, same_tile = a // 64 == b // 64, a // 128 == b // 128
                kinds |= {"lanes"} if same_half and b - a in (1, 4) else set()
                kinds |= {"registers"} if same_half and b - a == 16 else set()
                kinds |= {"halves"} if same_tile and not same_half else set()
                kinds |= {"tiles"} if not same_tile and b // 128 - a // 128 < 64 else set()
                kinds |= {"trip"} if (b // 128 - a // 128) % 64 == 0 and not same_tile else set()
                kinds |= {"one-tile"} if len(s) >= 9 and s[-1] // 128 == a // 128 else set()
                kinds |= {"nine-tiles"} if len({x // 128 for x in s}) >= 9 else set()
            want = {"lanes", "halves"} | ({"registers", "one-tile"} if c.K > 8 else set()) | ({"tiles", "trip", "nine-tiles"} if c.NT >= 65 else set())
            assert kinds >= want, (c.name, want - kinds)
            assert (r["argmax"] == np.array([sc.tie_sets(c.N)[p][0] for p in c.pat])).all()
    neg = [c for c in sc.all_cases() if c.cls in ("lit", "spread", "ties") and (c.ref()["zmax"] < 0).any()]
    assert len(neg) >= 10                                                   # negative maxima: an initial z[target] of 0 would win


def test_coverage_is_computed_from_the_mirrored_maps():
    for fam in ("mfma", "tall", "wide"):
        cols, rows = sc.tile_positions(fam)
        bm, bn = sc.BLOCK[fam]
        assert cols == set(range(bn)) and rows == set(range(bm)), fam     # the maps are onto the block tile
        alone, amax, tgt, rowpos, part = set(), set(), set(), set(), False
        for c in sc.all_cases():
            if sc.family(c.code(0)) != fam:
                continue
            rowpos |= {m % bm for m in range(c.M)}
            part |= c.M > bm and c.M % bm != 0
            tgt |= {int(t) % bn for t in c.targets}
            if c.cls not in ("lit", "ties"):
                continue
            z = c.z64().numpy()
            lit = z == z.max(1, keepdims=True)
            halves = np.zeros((c.M, c.NT * 2 * 64), dtype=bool)
            halves[:, :c.N] = lit
            only = halves.reshape(c.M, -1, 64).sum(2) == 1
            mm, nn = np.nonzero(lit)
            keep = only[mm, nn // 64]
            alone |= {int(n) % bn for n in nn[keep]}
            am = c.ref()["argmax"]
            amax |= {int(n) % bn for m, n in enumerate(am) if only[m, n // 64]}
        assert alone == set(range(bn)), (fam, sorted(set(range(bn)) - alone))
        assert amax == set(range(bn)), (fam, sorted(set(range(bn)) - amax))
        assert tgt == set(range(bn)), (fam, sorted(set(range(bn)) - tgt))
        assert rowpos == set(range(bm)) and part, fam
    # targets: lit, unlit, column 0, column N - 1, the argmax, a lit column of an upper half, a negative z in a ragged tile
    kinds = set()
    for c in sc.cases_of("lit"):
        r, t = c.ref(), c.targets
        lit = r["zt"] == r["zmax"]
        kinds |= {"lit"} if lit.any() else set()
        kinds |= {"unlit"} if (~lit).any() else set()
        kinds |= {"first"} if (t == 0).any() else set()
        kinds |= {"last"} if (t == c.N - 1).any() else set()
        kinds |= {"argmax"} if (t == r["argmax"]).any() else set()
        kinds |= {"upper"} if (lit & (t % 128 >= 64) & (t != r["argmax"])).any() else set()
        kinds |= {"negative-ragged"} if c.N % 128 and ((r["zt"] < 0) & (t // 128 == c.NT - 1)).any() else set()
        kinds |= {"one-column-tile"} if c.N % 128 == 1 and ((t == c.N - 1) & (r["argmax"] == c.N - 1)).any() else set()
    assert kinds == {"lit", "unlit", "first", "last", "argmax", "upper", "negative-ragged", "one-column-tile"}, kinds


def test_the_float32_chain_passes_and_sets_the_recorded_distance():
    worst, where = 0.0, None
    for c in sc.all_cases():
        for wt in c.wts[:1]:
            for k in (0, c.ks[-1]):
                out = c.chain(k, wt)
                ok, fig = c.judge(out, k)
                assert ok, (c.name, k, fig)
                if fig["d_lse"] > worst:
                    worst, where = fig["d_lse"], c.name
    print(f"float32 chain vs float64 reference: worst |d lse| {worst:.3e} ({where})")
    assert 0.5 * sc.MEASURED_F32_LSE <= worst <= 1.25 * sc.MEASURED_F32_LSE, (worst, where)
    assert where == sc.MEASURED_F32_LSE_CASE
    assert 2 * sc.MEASURED_F32_LSE < sc.LSE_BAR == 2e-5


def test_both_epilogue_orders_and_float64_of_the_chain_agree_with_the_reference():
    c = next(x for x in sc.cases_of("grid") if x.N == 8200)
    for fam in ("mfma", "tall"):
        for dtype in (np.float32, np.float64):
            ok, fig = c.judge(c.chain(8, 0, dtype=dtype, fam=fam), 8)
            assert ok, (fam, dtype, fig)
    a, b = c.chain(0, 0, fam="mfma"), c.chain(0, 0, fam="tall")
    assert not np.array_equal(a["lse"], b["lse"])                          # (the orders are different orders)


@pytest.mark.parametrize("mutation", sc.MUTATIONS)
def test_a_mutant_is_rejected(mutation):
    """the chain with one fault, judged as a device result: rejected by at least one case of EVERY kernel family (a fault may sit in one
    epilogue only); per family the smallest case that rejects it is printed"""
    for fam in ("mfma", "tall", "wide"):
        for c in _by_size():
            if sc.family(c.code(0)) != fam:
                continue
            k = c.ks[-1]
            ok, fig = c.judge(c.chain(k, 0, dtype=np.float64, mutate=mutation), k)
            if not ok:
                why = ", ".join(f"{a} {b if isinstance(b, bool) else format(b, '.2e')}" for a, b in fig.items() if b is False or (a == "d_lse" and b > sc.LSE_BAR))
                print(f"{mutation} [{fam}]: rejected by {c.name} (k = {k}): {why}")
                break
        else:
            raise AssertionError(f"no {fam} case rejects {mutation}")


def test_mutation_list_and_record_documentation():
    assert len(sc.MUTATIONS) == len(set(sc.MUTATIONS)) == 13
    kh = (ROOT / "detikzify_amd" / "csrc" / "kernels.h").read_text()
    assert re.search(r"7 the log-softmax epilogue \(launch_gemm_logsoftmax", kh) and "launch_gemm_logsoftmax does not set it" not in kh
    src = (ROOT / "detikzify_amd" / "csrc" / "kernels_batched.hip").read_text()
    body = src[src.index("bool launch_gemm_logsoftmax("):src.index("__global__ __launch_bounds__(64) void k_score_merge")]
    assert body.count("gemm_record(GEMM_KCODE(7,") == 2
