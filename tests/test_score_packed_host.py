"""The host side of packed candidate scoring (no GPU): the planner that splits candidates into passes, and the C ABI's additions
(declared in include/dtk.h, listed in _lib.SYMBOLS, ABI still 7)."""
from __future__ import annotations

import re
from pathlib import Path

import pytest

from detikzify_amd import _lib
from detikzify_amd.model.packing import plan_packed_passes

ROOT = Path(__file__).resolve().parent.parent
NEW = ("dtk_score_packed", "dtk_score_packed_text", "dtk_op_attention_seg")


def _fits(P, lens, passes, capacity):
    return all(P - 1 + sum(lens[i] for i in members) <= capacity for members in passes)


def test_one_pass_when_everything_fits():
    assert plan_packed_passes(10, [5, 6, 7], 100) == [[0, 1, 2]]


def test_single_candidate():
    assert plan_packed_passes(10, [20], 29) == [[0]]


def test_exact_fit_and_one_token_more():
    # P - 1 + sum = 9 + 5 + 6 + 7 = 27
    assert plan_packed_passes(10, [5, 6, 7], 27) == [[0, 1, 2]]
    assert plan_packed_passes(10, [5, 6, 7], 26) == [[0, 1], [2]]
    # a single candidate: exact fit, then exceeded by 1
    assert plan_packed_passes(10, [17], 26) == [[0]]
    with pytest.raises(ValueError, match="candidate 0"):
        plan_packed_passes(10, [18], 26)


def test_one_token_prompt_leaves_every_row_to_the_candidates():
    # P = 1: no prompt row is shared, the candidates may fill max_positions exactly
    assert plan_packed_passes(1, [10, 6], 16) == [[0, 1]]
    assert plan_packed_passes(1, [10, 7], 16) == [[0], [1]]
    assert plan_packed_passes(1, [16], 16) == [[0]]
    with pytest.raises(ValueError, match="candidate 0"):
        plan_packed_passes(1, [17], 16)


def test_greedy_in_input_order():
    P, lens, cap = 4, [30, 30, 50, 10, 60, 1, 1], 3 + 60
    passes = plan_packed_passes(P, lens, cap)
    assert passes == [[0, 1], [2, 3], [4], [5, 6]]       # a later, smaller candidate never jumps ahead to fill a pass
    assert [i for members in passes for i in members] == list(range(len(lens)))
    assert _fits(P, lens, passes, cap)


def test_six_candidates_in_three_passes():
    P, lens, cap = 21, [40, 41, 39, 42, 40, 38], 20 + 82
    passes = plan_packed_passes(P, lens, cap)
    assert passes == [[0, 1], [2, 3], [4, 5]] and _fits(P, lens, passes, cap)


def test_oversized_and_empty_candidates_raise():
    with pytest.raises(ValueError, match="candidate 1"):
        plan_packed_passes(10, [5, 92, 5], 100)
    with pytest.raises(ValueError, match="empty"):
        plan_packed_passes(10, [5, 0], 100)
    with pytest.raises(ValueError):
        plan_packed_passes(0, [5], 100)
    with pytest.raises(ValueError):
        plan_packed_passes(200, [1], 100)          # the prompt alone is over the capacity


def test_planner_is_reexported_by_the_model_module():
    from detikzify_amd.model import modeling
    assert modeling.plan_packed_passes is plan_packed_passes
    assert callable(getattr(modeling.DetikzifyForCausalLM, "score_candidates"))


def test_header_declares_the_functions_and_symbols_list_them():
    header = (ROOT / "include" / "dtk.h").read_text()
    for name in NEW:
        assert re.search(rf"^int\s+{name}\(", header, re.M), name
        assert name in _lib.SYMBOLS, name
    assert len(_lib.SYMBOLS["dtk_score_packed"][1]) == 12
    assert len(_lib.SYMBOLS["dtk_score_packed_text"][1]) == 15
    assert len(_lib.SYMBOLS["dtk_op_attention_seg"][1]) == 12


def test_abi_version_is_still_7():
    header = (ROOT / "include" / "dtk.h").read_text()
    assert re.search(r"#define\s+DTK_ABI_VERSION\s+7\b", header)
    assert _lib.DTK_ABI_VERSION == 7
