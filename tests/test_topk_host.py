"""Top-k alternatives, host side (no GPU): the additive C ABI (include/dtk.h "Top-k alternatives"), the Python argument checks —
which run before any library call — the batch engines' refusal, and the ordering helper the GPU tests compare the kernels with."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from detikzify_amd.infer.batching import BatchEngine
from detikzify_amd.infer.engine import NativeBatchEngine
from detikzify_amd.infer.generate import DetikzifyGenerator
from detikzify_amd.infer.pipeline import DetikzifyPipeline
from detikzify_amd.model.modeling import DetikzifyForCausalLM, GenerateOutput, check_top_logprobs

from .helpers import fake_processor
from .test_generate_loop import EOS, IMG, NIMG, VOCAB, ScriptedDevice, _prompt

NEW = ("dtk_score_top", "dtk_score_top_text", "dtk_score_packed_top", "dtk_score_packed_top_text", "dtk_op_score_top",
       "dtk_decode_wait_top", "dtk_decode_batch_wait_top")


def ordered_topk(z, k):
    """the first k ids of one row of logits ordered by z descending, token id ascending on exact ties (a stable sort of -z), and
    their z: what every top-k output of the library must equal"""
    z = np.asarray(z)
    order = np.argsort(-z.astype(np.float64), kind="stable")[:k]
    return order.astype(np.int64), z[order]


def test_ordering_helper_on_a_row_with_ties():
    z = np.array([1.0, 3.0, 3.0, -2.0, 3.0, 0.5, 1.0, -np.inf], dtype=np.float32)
    ids, vals = ordered_topk(z, 6)
    assert ids.tolist() == [1, 2, 4, 0, 6, 5] and vals.tolist() == [3.0, 3.0, 3.0, 1.0, 1.0, 0.5]
    assert ordered_topk(z, 1)[0].tolist() == [1]
    assert ordered_topk(z, 8)[0].tolist() == [1, 2, 4, 0, 6, 5, 3, 7]


def test_abi_is_additive():
    header = (Path(__file__).resolve().parents[1] / "include" / "dtk.h").read_text()
    lib = _lib.load_library()
    assert re.search(r"^#define DTK_MAX_TOP 8\b", header, re.M) and _lib.DTK_MAX_TOP == 8
    assert re.search(r"^#define DTK_ABI_VERSION 7\b", header, re.M) and lib.dtk_abi_version() == 7 == _lib.DTK_ABI_VERSION
    for name in NEW:
        assert re.search(r"^int\s+%s\(" % name, header, re.M), f"{name} is not declared in dtk.h"
        assert name in _lib.SYMBOLS and getattr(lib, name).argtypes is not None


class NoLibrary:
    """a model whose every library call fails the test: the argument checks must come first"""
    _weights_ready = True

    def __getattr__(self, name):
        raise AssertionError(f"{name} touched before the arguments were checked")


@pytest.mark.parametrize("k", [0, 9, -1])
def test_k_outside_1_to_8_is_refused_before_any_library_call(k):
    ids = torch.arange(6)
    with pytest.raises(ValueError, match="top_logprobs"):
        DetikzifyForCausalLM.score(NoLibrary(), ids, None, top_logprobs=k)
    with pytest.raises(ValueError, match="top_logprobs"):
        DetikzifyForCausalLM.score_candidates(NoLibrary(), ids, [ids], top_logprobs=k)
    with pytest.raises(ValueError, match="top_logprobs"):
        DetikzifyForCausalLM.generate(NoLibrary(), input_ids=ids[None], return_logprobs=True, top_logprobs=k)
    with pytest.raises(ValueError, match="top_logprobs"):
        DetikzifyPipeline.sample(NoLibrary(), image=object(), return_logprobs=True, top_logprobs=k)
    with pytest.raises(ValueError, match="top_logprobs"):
        DetikzifyPipeline.score(NoLibrary(), image=object(), code="x", top_logprobs=k)
    with pytest.raises(ValueError, match="top_logprobs"):
        DetikzifyGenerator.sample(NoLibrary(), return_logprobs=True, top_logprobs=k)


def test_top_logprobs_needs_return_logprobs():
    ids = torch.arange(6)
    with pytest.raises(ValueError, match="return_logprobs"):
        DetikzifyForCausalLM.generate(NoLibrary(), input_ids=ids[None], top_logprobs=3)
    with pytest.raises(ValueError, match="return_logprobs"):
        DetikzifyPipeline.sample(NoLibrary(), image=object(), top_logprobs=3)
    with pytest.raises(ValueError, match="return_logprobs"):
        DetikzifyGenerator.sample(NoLibrary(), top_logprobs=3)
    assert check_top_logprobs(None, False) == 0 and check_top_logprobs(8) == 8 and check_top_logprobs(1) == 1


@pytest.mark.parametrize("make", [NativeBatchEngine, BatchEngine], ids=lambda m: m.__name__)
def test_the_batch_engines_refuse(make):
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 1)
    dev = ScriptedDevice(slots=5)
    eng = make(dev, max_batch=4)
    try:
        with pytest.raises(NotImplementedError, match="top_logprobs: not in the batch engines yet"):
            with eng.sequence(ids, px, dict(do_sample=False), max_new_tokens=4, top_logprobs=3):
                pass
        with pytest.raises(NotImplementedError, match="top_logprobs: not in the batch engines yet"):
            dev.generate(input_ids=ids[None], pixel_values=px, seed=1, return_logprobs=True, top_logprobs=3,
                         bad_words_ids=[[IMG]], begin_suppress_tokens=[EOS], do_sample=True, max_length=NIMG + 20)
    finally:
        eng.close()


def test_generate_output_carries_the_two_fields():
    out = GenerateOutput(torch.zeros(1, 3), torch.zeros(1, 2), torch.zeros(1, 2))
    assert out.top_ids is None and out.top_logprobs is None
