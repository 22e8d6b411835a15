"""The host side of the decode-attention op tests (no GPU): the float64 reference against the oracle's attention, the spotlight
input builder — every input tests/test_gpu_attn_decode.py feeds to the kernels is built here too, so its >= 0.99-mass assertion runs
on a machine without a GPU —, that a one-key error in the reference is far outside the bar, and the C ABI's additions."""
from __future__ import annotations

import re
from pathlib import Path

import pytest
import torch

from detikzify_amd import _lib
from oracle.llama import attention
from oracle.ops import f32_to_bits, rb
from tests import attn_decode_cases as ac
from tests.helpers import rel_l2

ROOT = Path(__file__).resolve().parent.parent
NEW = ("dtk_op_attn_decode", "dtk_op_attn_decode_b")


def _ulps(got, ref):
    """test_op_attention's measure of two fp32 tensors that hold bf16 values"""
    got, ref = got.reshape(-1).float(), rb(ref.float()).reshape(-1)
    ulp = torch.clamp(ref.abs(), min=1e-2 * float(ref.abs().max()) + 1e-30) * 2.0 ** -7
    return float(((got - ref).abs() / ulp).max()), rel_l2(got, ref)


@pytest.mark.parametrize("hd,KVH", [(128, 8), (128, 2), (64, 8), (64, 2)])
def test_reference_is_the_oracles_attention_at_one_query(hd, KVH):
    """float64 against the oracle's fp32 softmax: one bf16 rounding flip at the most"""
    case = ac.single_random_case(hd, KVH)
    for i, p in enumerate(case.positions):
        want = attention(case.q[:, None, :], case.K[:, :p + 1], case.V[:, :p + 1], hd ** -0.5)[:, 0]
        ulps, rl2 = _ulps(want, case.ref[i])
        assert ulps <= 1.01 and rl2 < 1e-3, (p, ulps, rl2)


@pytest.mark.parametrize("hd,KVH", [(128, 8), (128, 2), (64, 8), (64, 2)])
def test_single_sequence_spotlights_hold_their_mass(hd, KVH):
    """every (threads, splits) the GPU test runs: the builder asserts >= 0.99 itself; here also that every kind of spotlight the
    issue names occurs, that V rows are distinct and that the poison is finite"""
    seen = {}
    for threads in sorted({t for t, _ in (ac.CONFIGS_128 if hd == 128 else ac.CONFIGS_64)}):
        for S in ac.SPLITS:
            for case in ac.single_cases(hd, KVH, threads, S):
                for k, v in case.wants().items():
                    seen[(threads, S, k)] = seen.get((threads, S, k), 0) + int(v)
                assert torch.isfinite(case.K).all() and torch.isfinite(case.V).all() and torch.isfinite(case.K2).all()
                top = max(case.positions)
                assert len({tuple(r.tolist()) for r in case.V[0, :top + 1]}) == top + 1
                if top + 1 < ac.T_MAX:
                    assert float(case.K[:, top + 1:].abs().min()) > 2e4 and not torch.equal(case.K[:, top + 1:], case.K2[:, top + 1:])
                    assert torch.equal(f32_to_bits_t(case.K[:, :top + 1]), f32_to_bits_t(case.K2[:, :top + 1]))
    for (threads, S, kind), n in seen.items():
        assert n > 0 or (kind == "split2" and S == 1), (threads, S, kind)


def f32_to_bits_t(x):
    return torch.from_numpy(f32_to_bits(x).astype("int32"))


@pytest.mark.parametrize("KVH", [8, 4, 2])
def test_batched_spotlights_hold_their_mass(KVH):
    for rows in (16, 32, 64, 128):
        case = ac.unshared_case(KVH, rows)
        assert case.active[3] == 0 and case.active[9] == 0 and sum(case.active) == 14
        assert {h for (_, h) in case.spots} == {0, 1, 2}
        cases = ac.shared_cases(KVH, rows)
        forks = {(c.L[s], c.pos[s] + 1 - c.L[s]) for c in cases for s in range(1, c.n) if c.active[s]}
        assert {L for L, _ in forks} == set(ac.B_SHARE_LENS)
        assert {n for _, n in forks} >= {n for n in ac.private_lengths(rows) if n >= 1 and 3 + n <= ac.B_T_MAX}
        for c in cases:
            assert torch.isfinite(c.K).all() and torch.isfinite(c.V).all()
            for s in range(1, c.n):
                if c.active[s]:
                    assert {h for (t, h) in c.spots if t == s} == {0, 1, 2, 3}
                    assert float(c.K[s, :, :c.L[s]].abs().min()) > 2e4          # a fork's own rows below L are poison


def test_grouping_case_layout():
    c = ac.grouping_case()
    assert sum(1 for s in range(64) if c.active[s] and c.src[s] == 0) == 17
    assert sum(1 for s in range(64) if c.active[s] and c.src[s] == 20) == 2
    assert c.active[24] and c.src[25] == 24 and not c.active[0] and not c.active[20]
    assert sum(1 for s in range(64) if c.active[s] and c.src[s] < 0 and s != 24) == 6


def test_a_one_key_error_is_far_outside_the_bar():
    """the reference over keys 0..pos-1 instead of 0..pos, and a fork over its own rows instead of its source's, measured with the
    GPU test's bar against the true reference: every spotlit head must miss it — so a kernel with that error could not pass"""
    case = ac.single_cases(128, 2, 256, 4)[0]
    for i, p in enumerate(case.positions):
        if p == 0:
            continue
        wrong = ac.attn_ref(case.q, case.K, case.V, p - 1)[0]
        ulps, rl2 = _ulps(rb(wrong.float()), case.ref[i])
        assert ulps > 4.01 and rl2 > 2e-3, (p, ulps, rl2)
        assert _ulps(rb(wrong.float())[0], case.ref[i][0])[0] > 4.01            # head 0 spotlights key pos
    c = ac.shared_cases(4, 64)[0]
    for s in range(1, c.n):
        if c.active[s]:
            ulps, rl2 = _ulps(rb(c.own_rows_ref(s).float()), c.ref[s])
            assert ulps > 4.01 and rl2 > 2e-3, (s, ulps, rl2)


def test_combine_partials_of_one_split_is_the_identity():
    pm, pl, po = torch.tensor([[0.5, -1e30]]), torch.tensor([[2.0, 0.0]]), torch.tensor([[[4.0, 6.0], [0.0, 0.0]]])
    assert torch.equal(ac.combine_partials(pm, pl, po), torch.tensor([[2.0, 3.0]], dtype=torch.float64))


def test_header_declares_the_functions_and_symbols_list_them():
    header = (ROOT / "include" / "dtk.h").read_text()
    for name in NEW:
        assert re.search(rf"^int\s+{name}\(", header, re.M), name
        assert name in _lib.SYMBOLS, name
    assert len(_lib.SYMBOLS["dtk_op_attn_decode"][1]) == 18
    assert len(_lib.SYMBOLS["dtk_op_attn_decode_b"][1]) == 18
    assert re.search(r"#define\s+DTK_ABI_VERSION\s+7\b", header) and _lib.DTK_ABI_VERSION == 7
