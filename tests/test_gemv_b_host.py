"""The host side of the batched decode GEMV op tests (no GPU): every input tests/test_gpu_gemv_b.py feeds to the kernels is built here
too; the float64 reference against oracle/llama.py in float32 end to end (their worst distance sets the bar of the chained outputs);
each deliberately wrong reference misses the bar at every case it applies to; the C ABI's additions."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

from detikzify_amd import _lib
from tests import gemv_b_cases as gc

ROOT = Path(__file__).resolve().parent.parent
NEW = ("dtk_op_gemv_b", "dtk_op_gemv_bkp")


def test_inputs_are_what_the_issue_asks_for():
    assert sorted(gc.POS) == list(range(gc.T_MAX)) and gc.POS[0] == gc.T_MAX - 1 and gc.POS[1] == 0 and gc.POS[2] == gc.T_MAX - 2
    lay = gc.active_sets(64)
    assert [s for s, a in enumerate(lay["interleaved"]) if not a] == list(gc.IDLE)
    assert not any(lay["idle_tile"][16:32]) and sum(lay["one_slot"]) == 1
    assert gc.active_sets(1)["interleaved"] == [1]
    names = set()
    for c in gc.all_cases():
        assert c.name not in names, c.name
        names.add(c.name)
        assert len({tuple(r.tolist()) for r in c.X}) == gc.SLOTS                  # every slot its own x
        if c.fmt == "fp8":
            e = np.log2(c.wscale.numpy())
            assert (e == np.round(e)).all() and (e.max() - e.min() >= 6 or c.N < 7)
            for gap in (1, 16, 64) + ((c.ff,) if c.epi == gc.SWIGLU else ()):     # neighbours, row tiles, RoPE / gate-up partners
                if gap < c.N:
                    assert (e[gap:] != e[:-gap]).all(), (c.name, gap)
        for bufs in (c.initial(lay["interleaved"]),):
            for name, b in bufs.items():
                idle = np.isnan(gc.bits_to_f32(b).numpy()) if b.dtype == np.uint16 else np.isnan(b)
                assert idle.all() or (c.epi in (gc.RESID, gc.BKP) and name == "y" and idle[list(gc.IDLE)].all()), (c.name, name)
    # every shape and format of the issue's lists
    want = {f"{e}-{shape}-K{K}-{fmt}" for K in gc.SMALL_K for fmt in ("bf16", "fp8")
            for e, shape in (("logits", "N77"), ("logits", "N130"), ("resid", "N144"), ("resid", "N200"), ("swiglu", "ff24"), ("swiglu", "ff88"),
                             ("qkv", "H2KVH1"), ("qkv", "H2KVH2"))}
    assert want <= {n.replace("-norm", "").replace("-grid", "") for n in names}
    assert {"resid-N256-K72-bf16", "resid-N224-K72-bf16", "resid-N256-K72-bf16-grid", "qkv-H2KVH1-K256-bf16-norm", "qkv-H2KVH2-K304-fp8"} <= names
    for K in (2048, 4096):
        assert {f"{r}-K{K}-{fmt}{g}" for g in ("", "-grid") for fmt in ("bf16", "fp8") for r in ("qkv-H2KVH1", "qkv-H2KVH2", "swiglu-ff80", "swiglu-ff96", "logits-N160",
                                                                       "logits-N192")} <= names
    assert {f"bkp-N{N}-K{K}-{fmt}" for N in (2048, 4096) for K in (256, 480, 768) for fmt in ("bf16", "fp8")} <= names
    assert {f"bkp-N{N}-K{K}-{fmt}-grid" for N, K in ((2048, 256), (2048, 480), (4096, 768)) for fmt in ("bf16", "fp8")} <= names


def test_reference_against_the_float32_oracle_and_the_bar_it_sets():
    """the float32 chain run through the buffers and judged like a device result passes everywhere; the worst distance of the chained
    outputs is what tests/gemv_b_cases.py records, and the GPU bar is twice it under the caps"""
    wu = wr = raw = 0.0
    for c in gc.all_cases():
        if c.epi == gc.QKV and not c.grid:
            raw = max(raw, c.raw_rope_distance())
        far = c.reference("f32")
        for nslots, layout, act in gc.runs(c):
            ok, fig = c.judge(c.written(far, act), act)
            assert ok, (c.name, nslots, layout, fig)
        u, r = c.reference_distance()
        wu, wr = max(wu, u), max(wr, r)
    print(f"float64 vs float32 reference, chained outputs: worst {wu:.2f} ulps, rel-L2 {wr:.2e}")
    # (the float32 matmul's summation order belongs to the BLAS at hand: the recorded figures may move a little, not by a factor)
    assert 0.5 * gc.MEASURED_CHAIN_ULPS <= wu <= 1.25 * gc.MEASURED_CHAIN_ULPS, wu
    assert 0.5 * gc.MEASURED_CHAIN_RL2 <= wr <= 1.25 * gc.MEASURED_CHAIN_RL2, wr
    # q / k after RoPE on random operands in ulps of the element: the two legitimate references are further apart than the cap
    print(f"q / k on random operands in ulps of the element: {raw:.2f}")
    assert 0.8 * gc.RAW_ROPE_ULPS <= raw <= 1.25 * gc.RAW_ROPE_ULPS and gc.RAW_ROPE_ULPS > 4.01, raw
    assert gc.CHAIN_ULPS == min(4.01, 2 * gc.MEASURED_CHAIN_ULPS) and gc.CHAIN_RL2 == min(2e-3, 2 * gc.MEASURED_CHAIN_RL2)
    assert (gc.SINGLE_RL2, gc.SINGLE_ULPS, gc.SINGLE_FRAC) == (1e-3, 2.01, 0.05)


@pytest.mark.parametrize("mutation", gc.MUTATIONS)
def test_a_wrong_reference_misses_the_bar(mutation):
    """slot s reads slot s ^ 1's x; pos off by one; the RoPE partner's sign flipped; gate and up swapped; one k-step of 32 dropped /
    counted twice; the last partial k-step dropped; the scale of row r + 1 / r - 1; res + p rounded once (GRID cases: on random
    operands that is at most one ulp, which no ulp bar sees) — judged as a device result, in every run of every case it applies to"""
    hit = 0
    for c in gc.all_cases():
        if not c.applies(mutation):
            continue
        wrong = c.reference(mutate=mutation)
        for nslots, layout, act in gc.runs(c):
            ok, fig = c.judge(c.written(wrong, act), act)
            assert not ok, (mutation, c.name, nslots, layout, fig)
            hit += 1
    assert hit > 0


def test_header_declares_the_functions_and_symbols_list_them():
    header = (ROOT / "include" / "dtk.h").read_text()
    for name in NEW:
        assert re.search(rf"^int\s+{name}\(", header, re.M), name
        assert name in _lib.SYMBOLS, name
        decl = re.search(rf"^int\s+{name}\((.*?)\);", header, re.M | re.S).group(1)
        assert len(_lib.SYMBOLS[name][1]) == decl.count(",") + 1, name
    assert len(_lib.SYMBOLS["dtk_op_gemv_b"][1]) == 28
    assert len(_lib.SYMBOLS["dtk_op_gemv_bkp"][1]) == 15
    assert re.search(r"#define\s+DTK_ABI_VERSION\s+7\b", header) and _lib.DTK_ABI_VERSION == 7
    table = (ROOT / "INTEGRATION.md").read_text()
    assert all(name in table for name in NEW)
