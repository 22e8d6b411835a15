"""Host side of teacher-forced scoring (model.score / model.forward(labels=...) / dtk_score): the loss reduction against torch's
CrossEntropyLoss on the reference's own all-position logits, the C-ABI additions, and forward()'s argument gate.  No GPU."""
from __future__ import annotations

import re
import threading
from pathlib import Path

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from detikzify_amd.model.modeling import DetikzifyForCausalLM, GenerationConfig, shifted_cross_entropy
from tests.helpers import TINY, top2_gap_ulps

GOLDEN = Path(__file__).resolve().parent / "golden"
HEADER = Path(__file__).resolve().parents[1] / "include" / "dtk.h"


def _golden_logprobs(name):
    g = np.load(GOLDEN / name)
    logits, ids = torch.from_numpy(g["prefill_logits"]).float(), torch.from_numpy(g["ids"]).to(torch.int64)
    assert logits.shape[0] == ids.numel() == 15
    lp = torch.log_softmax(logits, dim=-1)[:-1].gather(1, ids[1:, None])[:, 0]
    return logits, ids, lp


@pytest.mark.parametrize("name", ["reference_v1_tiny.npz", "reference_v2_tiny.npz"])
def test_loss_reduction_is_torch_cross_entropy_on_the_reference_logits(name):
    logits, ids, lp = _golden_logprobs(name)
    ce = torch.nn.CrossEntropyLoss()
    loss = shifted_cross_entropy(lp, ids, first=1)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    torch.testing.assert_close(loss, ce(logits[:-1], ids[1:]))
    # some positions ignored (the prompt part of a (figure, TikZ) pair is labelled -100)
    for masked in ([0, 1, 2, 3], [5, 9], [14], list(range(0, 12))):
        labels = ids.clone()
        labels[masked] = -100
        torch.testing.assert_close(shifted_cross_entropy(lp, labels, first=1), ce(logits[:-1], labels[1:]))
    # a scoring pass that starts later: first = 6 with labels[:6] ignored
    labels = ids.clone()
    labels[:6] = -100
    torch.testing.assert_close(shifted_cross_entropy(lp[5:], labels, first=6), ce(logits[:-1], labels[1:]))
    with pytest.raises(ValueError):
        shifted_cross_entropy(lp[5:], ids, first=6)          # a kept label whose log-probability was not computed
    with pytest.raises(ValueError):
        shifted_cross_entropy(lp[:-1], ids, first=1)
    # nothing kept: NaN, as torch
    none = torch.full_like(ids, -100)
    assert torch.isnan(ce(logits[:-1], none[1:])) and torch.isnan(shifted_cross_entropy(lp, none, first=1))


@pytest.mark.parametrize("name", ["reference_v1_tiny.npz", "reference_v2_tiny.npz"])
def test_reference_near_ties_stay_within_a_quarter(name):
    """the condition the GPU tests' argmax exemption rests on, counted from the committed goldens alone (raw logits, no masks)"""
    g = np.load(GOLDEN / name)
    rows = [("prefill", torch.from_numpy(g["prefill_logits"]).float()[:-1]), ("step", torch.from_numpy(g["step_logits"]).float())]
    for tag, lg in rows:
        near = sum(top2_gap_ulps(r, [], [], False) <= 2.0 for r in lg)
        print(f"{name} {tag}: {near} of {lg.shape[0]} rows within 2 bf16 ulps")
        assert 4 * near <= lg.shape[0]


def test_c_abi_declares_and_binds_the_scoring_entry_points():
    text = HEADER.read_text()
    for name in ("dtk_score", "dtk_score_text", "dtk_op_score"):
        assert name in _lib.SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert _lib.DTK_ABI_VERSION == 7 and re.search(r"#define\s+DTK_ABI_VERSION\s+7\b", text)
    # dtk_score's argument list as include/dtk.h states it
    res, args = _lib.SYMBOLS["dtk_score"]
    assert len(args) == 10 and len(_lib.SYMBOLS["dtk_score_text"][1]) == 13


def _deviceless_model():
    m = DetikzifyForCausalLM.__new__(DetikzifyForCausalLM)
    m.config, m.batch_engine, m._weights_ready, m.reuse_prefix = TINY, None, True, False
    m.generation_config = GenerationConfig(eos_token_id=2)
    m._vit_lock, m._single_busy, m._ctx, m.lib = threading.RLock(), threading.Lock(), None, None
    return m


def test_forward_gate_without_a_device():
    m = _deviceless_model()
    ids = torch.tensor([[1, 5, 6, 7]])
    with pytest.raises(NotImplementedError, match=r"prefill\(.*return_logits=True\)"):
        m.forward(input_ids=ids, labels=None)
    with pytest.raises(NotImplementedError, match=r"prefill\(.*return_logits=True\)"):
        m(input_ids=ids, labels=ids, output_logits=True)
    with pytest.raises(TypeError, match="forward"):
        m(input_ids=ids, labels=ids, no_such_argument=1)
    with pytest.raises(NotImplementedError):
        m(input_ids=ids, labels=ids, output_attentions=True)      # a name forward() shares with generate(): the same gate
    for generate_only in (dict(num_beams=1), dict(max_new_tokens=None), dict(streamer=None), dict(pad_token_id=0)):
        with pytest.raises(TypeError, match="forward"):           # neutral for generate(), but not an argument of forward()
            m(input_ids=ids, labels=ids, **generate_only)
    with pytest.raises(ValueError, match="adapter_attention_mask"):
        m.score(ids, adapter_attention_mask=torch.ones(1, 3))
    with pytest.raises(NotImplementedError):
        m(input_ids=ids, labels=ids, return_dict=False)
    with pytest.raises(ValueError):
        m(input_ids=ids, labels=torch.tensor([[1, 5, 6]]))
    with pytest.raises(NotImplementedError):
        m(input_ids=ids, labels=torch.tensor([[-100, 5, 9, 7]]))  # a kept label that is not the input id
    out = m(input_ids=ids, labels=torch.full_like(ids, -100), use_cache=False, return_dict=True, attention_mask=torch.ones_like(ids))   # nothing to score: no device call
    assert torch.isnan(out.loss) and out.loss.dtype == torch.float32 and out.logits is None


def test_score_is_refused_while_a_batch_engine_is_busy():
    m = _deviceless_model()
    m.batch_engine = type("E", (), {"busy": lambda self: True})()
    with pytest.raises(_lib.DtkError, match="score"):
        m.score(torch.tensor([1, 5, 6, 7]))
    m._weights_ready = False
    with pytest.raises(_lib.DtkError, match="no weights"):
        m.score(torch.tensor([1, 5, 6, 7]))
