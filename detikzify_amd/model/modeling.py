"""
The (model, processor) pair's model half: an object with the attribute surface DeTikZify's
inference code touches, over the C ABI of libdtk_hip.so.

Replaces (reference, all Python): DetikzifyForCausalLM / DetikzifyModel / DetikzifyVisionModel
(detikzify/model/v1/modeling_detikzify.py:49-305) and the HF GenerationMixin.generate loop they
inherit (called at detikzify/infer/generate.py:218-227).  Surface kept:
  model.generate(input_ids, bad_words_ids, begin_suppress_tokens, pixel_values, streamer,
                 stopping_criteria, temperature, top_p, top_k, max_length, do_sample, ...)
  model.device / .dtype / .name_or_path / .generation_config.to_dict() / .config.{image_token_id,
  text_config.eos_token_id, pooling_mode} / model.model.vision_model(pixel_values=...)
There is no CPU fallback: constructing the model without the HIP library or a GPU raises.
"""
from __future__ import annotations

import math
import threading
import ctypes as C
import hashlib
from types import SimpleNamespace
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import _lib
from .config import DetikzifyConfig
from .packing import plan_packed_passes


class GenerationConfig:
    """transformers.GenerationConfig stand-in: only `.to_dict()` and attribute reads are used
    (infer/generate.py:211; v1/__init__.py:41)."""

    def __init__(self, **kw):
        self.max_length = 20           # HF default; the pipeline overrides it (generate.py:383)
        self.max_new_tokens = None
        self.do_sample = False
        self.temperature = 1.0
        self.top_p = 1.0
        self.top_k = 50
        self.eos_token_id = None
        self.pad_token_id = None
        self.bos_token_id = None
        self.__dict__.update(kw)

    def to_dict(self) -> Dict[str, Any]:
        return dict(self.__dict__)

    def update_from_dict(self, values: Dict[str, Any]) -> None:
        """generation_config.json of a checkpoint (what from_pretrained loads into model.generation_config); bookkeeping
        keys ("_from_model_config", "transformers_version") are dropped"""
        self.__dict__.update({k: v for k, v in values.items() if not k.startswith("_") and k != "transformers_version"})


class VisionOutput(SimpleNamespace):
    """BaseModelOutputWithPoolingAndNoAttention stand-in (last_hidden_state, pooler_output)."""


class DetikzifyVisionModel:
    """model.model.vision_model: timm ViT forward_features + forward_head on the GPU
    (reference v1/modeling_detikzify.py:63-69)."""

    def __init__(self, owner: "DetikzifyForCausalLM"):
        self._owner = owner
        self._pool_lock = threading.Lock()
        self._pool_queue: List[Any] = []        # [pixels, done event, result | exception] of threads waiting for a pooled output
        self._pool_leader = False

    def __call__(self, pixel_values: torch.Tensor, **_) -> VisionOutput:
        return self.forward(pixel_values)

    def forward(self, pixel_values: torch.Tensor) -> VisionOutput:
        feats, pooled = self._owner.vit_encode(pixel_values, want_pooled=True)
        return VisionOutput(last_hidden_state=feats, pooler_output=pooled)

    def pooled_only(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """pooler_output without copying the 729 x 1152 patch features back (SelfSim "cos": the reward's hot call).

        Calls that arrive from several threads at once (the trees of a parallel search scoring their rollouts) are combined:
        the first caller becomes the leader and encodes whatever has queued up — up to DTK_VIT_BATCH images per pass over the
        tower, 2.7 ms per image instead of 4.1 — until the queue is empty; the others sleep until their result is in.  Per image
        the result is bit-identical to a call of its own (dtk_vit_encode's batch rows are independent)."""
        px = pixel_values.detach().to("cpu", torch.float32)
        if px.dim() == 3:
            px = px[None]
        if px.shape[0] != 1:
            return self._owner.vit_encode(px, want_pooled=True, want_feats=False)[1]
        item = [px, threading.Event(), None]
        with self._pool_lock:
            self._pool_queue.append(item)
            lead = not self._pool_leader
            if lead:
                self._pool_leader = True
        if lead:
            while True:
                with self._pool_lock:
                    batch, self._pool_queue = self._pool_queue[:_lib.DTK_VIT_BATCH], self._pool_queue[_lib.DTK_VIT_BATCH:]
                    if not batch:
                        self._pool_leader = False
                        break
                try:
                    out = self._owner.vit_encode(torch.cat([it[0] for it in batch]), want_pooled=True, want_feats=False)[1]
                    for k, it in enumerate(batch):
                        it[2] = out[k:k + 1].clone()
                except BaseException as e:  # noqa: BLE001  (every waiter gets the error; the leader re-raises its own below)
                    for it in batch:
                        it[2] = e
                for it in batch:
                    it[1].set()
        item[1].wait()
        if isinstance(item[2], BaseException):
            raise item[2]
        return item[2]

    def get_intermediate_layers(self, pixel_values: torch.Tensor, *_, **__):
        feats, _ = self._owner.vit_encode(pixel_values, want_pooled=False)
        return [feats]


# HF generate() arguments this path does not implement, each with the value(s) at which HF's _sample does exactly what
# this loop does.  Passing one of them at such a value is harmless (the reference's callers and HF's own defaults do);
# any other value, and any name that is neither here nor a parameter of generate(), raises.
_NEUTRAL_GENERATE_KWARGS: Dict[str, tuple] = {
    "attention_mask": "any", "use_cache": "any", "pad_token_id": "any", "bos_token_id": "any", "synced_gpus": "any",
    "return_dict_in_generate": (None, False), "output_scores": (None, False), "output_logits": (None, False),
    "output_attentions": (None, False), "output_hidden_states": (None, False),
    "num_beams": (None, 1), "num_beam_groups": (None, 1), "num_return_sequences": (None, 1),
    "repetition_penalty": (None, 1.0), "encoder_repetition_penalty": (None, 1.0), "length_penalty": (None, 1.0),
    "diversity_penalty": (None, 0.0), "no_repeat_ngram_size": (None, 0), "encoder_no_repeat_ngram_size": (None, 0),
    "min_length": (None, 0), "typical_p": (None, 1.0),
    "eta_cutoff": (None, 0.0), "penalty_alpha": (None, 0.0), "early_stopping": (None, False),
    "renormalize_logits": (None, False), "remove_invalid_values": (None, False),
    "forced_bos_token_id": (None,), "forced_eos_token_id": (None,),
    "logits_processor": (None, [], ()), "prefix_allowed_tokens_fn": (None,),
    "assistant_model": (None,), "negative_prompt_attention_mask": (None,),
    "generation_config": (None,), "stop_strings": (None,), "max_time": (None,), "cache_implementation": (None,),
    "past_key_values": (None,), "inputs_embeds": (None,), "tokenizer": "any",
}


class GenerateOutput:
    """generate(return_logprobs=True): `.sequences` is what generate() returns without the flag; `.logprobs[0, i]` is the model's
    log-probability of new token i (z[t] - logsumexp(z) over the raw logits: what model.score reports for that position),
    `.sample_logprobs[0, i]` the log of the probability with which the sampler drew it (after the suppression lists, temperature,
    top-k and top-p; 0 for greedy).  Both [1, new_tokens] float32 on the CPU.  With top_logprobs=k also `.top_ids` (int64) and
    `.top_logprobs` (float32), [1, new_tokens, k]: the k most likely tokens of the raw logits each new token was sampled from, most
    likely first (lower id first on ties), and their log-probabilities; None without the argument."""

    def __init__(self, sequences: torch.Tensor, logprobs: torch.Tensor, sample_logprobs: torch.Tensor,
                 top_ids: Optional[torch.Tensor] = None, top_logprobs: Optional[torch.Tensor] = None):
        self.sequences, self.logprobs, self.sample_logprobs = sequences, logprobs, sample_logprobs
        self.top_ids, self.top_logprobs = top_ids, top_logprobs
        self.accepted_per_step: Optional[List[int]] = None      # prompt_lookup_num_tokens: tokens every speculative step accepted
        self.draft_sources: Optional[Tuple[int, int, int]] = None      # prompt_lookup_corpus: steps whose drafts came from (history, corpus, nowhere)


def check_prompt_lookup(prompt_lookup_num_tokens, max_matching_ngram_size=None) -> Tuple[int, int]:
    """the `prompt_lookup_num_tokens` / `max_matching_ngram_size` arguments of generate (HF's names and defaults) -> (K, n): K = 0 is
    off (None and 0); K in 1 .. 3 drafts per step, n in 1 .. 16 (default 2); ValueError before anything runs"""
    n = 2 if max_matching_ngram_size is None else max_matching_ngram_size
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= _lib.DTK_SPEC_MAX_NGRAM:
        raise ValueError(f"max_matching_ngram_size = {max_matching_ngram_size!r}: an integer in 1 .. {_lib.DTK_SPEC_MAX_NGRAM}")
    k = prompt_lookup_num_tokens
    if k is None:
        return 0, n
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= 3:
        raise ValueError(f"prompt_lookup_num_tokens = {prompt_lookup_num_tokens!r}: an integer in 1 .. 3 (the multi-vector step carries "
                         "at most 4 positions of one sequence; None / 0 = off)")
    return k, n


def flatten_corpus(seqs, vocab: int) -> List[int]:
    """the `prompt_lookup_corpus` argument of generate — 1-D id sequences, lists or tensors — as the flat corpus the device holds: the
    non-empty sequences in order, a -1 separator between two of them.  ValueError for an id outside [0, vocab), for anything that is
    not a 1-D sequence of integers, and when the ids plus their separators exceed DTK_SPEC_CORPUS_MAX"""
    if seqs is None:
        return []
    if isinstance(seqs, torch.Tensor) or (len(seqs) > 0 and isinstance(seqs[0], int)):
        raise ValueError("prompt_lookup_corpus: a list of 1-D id sequences (lists or tensors), not one sequence")
    flat: List[int] = []
    for seq in seqs:
        if isinstance(seq, torch.Tensor):
            if seq.dim() != 1 or seq.is_floating_point():
                raise ValueError(f"prompt_lookup_corpus: a 1-D tensor of ids per sequence, got shape {tuple(seq.shape)} of {seq.dtype}")
            seq = seq.tolist()
        seq = list(seq)
        if not seq:
            continue
        for t in seq:
            if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < vocab:
                raise ValueError(f"prompt_lookup_corpus: id {t!r} is outside [0, {vocab})")
        if flat:
            flat.append(-1)
        flat.extend(seq)
        if len(flat) > _lib.DTK_SPEC_CORPUS_MAX:
            raise ValueError(f"prompt_lookup_corpus: the sequences and their separators exceed {_lib.DTK_SPEC_CORPUS_MAX} entries")
    return flat


def check_top_logprobs(top_logprobs: Optional[int], return_logprobs: bool = True) -> int:
    """the `top_logprobs` argument of score / generate / sample -> k (0 = not asked for); ValueError before anything runs"""
    if top_logprobs is None:
        return 0
    if not return_logprobs:
        raise ValueError("top_logprobs needs return_logprobs=True")
    k = int(top_logprobs)
    if not 1 <= k <= _lib.DTK_MAX_TOP:
        raise ValueError(f"top_logprobs = {top_logprobs}: 1 .. {_lib.DTK_MAX_TOP}")
    return k


def check_guidance_scale(guidance_scale) -> float:
    """the `guidance_scale` argument of generate -> g (1.0 = off: None and 1); a finite real number in [0, 100], ValueError before
    anything runs"""
    if guidance_scale is None:
        return 1.0
    if isinstance(guidance_scale, bool) or not isinstance(guidance_scale, (int, float)):
        raise ValueError(f"guidance_scale = {guidance_scale!r}: a number in [0, 100]")
    g = float(guidance_scale)
    if not math.isfinite(g) or not 0.0 <= g <= 100.0:
        raise ValueError(f"guidance_scale = {guidance_scale!r}: a finite number in [0, 100]")
    return g


def check_truncation(min_p: Optional[float], epsilon_cutoff: Optional[float]) -> Tuple[float, float]:
    """the `min_p` / `epsilon_cutoff` arguments of generate / sample -> (min_p, epsilon_cutoff), 0.0 = off (None, and HF's own "unset");
    out of range: ValueError with the text of HF's MinPLogitsWarper / EpsilonLogitsWarper, before anything runs"""
    mp = 0.0 if min_p is None else min_p
    if not (isinstance(mp, (int, float)) and 0 <= mp <= 1.0):
        raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {min_p}")
    eps = 0.0 if epsilon_cutoff is None else epsilon_cutoff
    if not (isinstance(eps, (int, float)) and 0 <= eps < 1):
        raise ValueError(f"`epsilon_cutoff` has to be a float > 0 and < 1, but is {epsilon_cutoff}")
    return float(mp), float(eps)


def check_penalties(presence_penalty: Optional[float], frequency_penalty: Optional[float],
                    penalty_start: Optional[int] = None) -> Tuple[float, float, Optional[int]]:
    """the `presence_penalty` / `frequency_penalty` / `penalty_start` arguments of generate / sample -> (presence, frequency, start),
    0.0 = off (None); start None = the caller's default (generate: the prompt length).  Out of range: ValueError before anything runs"""
    out = []
    for name, v in (("presence_penalty", presence_penalty), ("frequency_penalty", frequency_penalty)):
        x = 0.0 if v is None else v
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not (-2.0 <= x <= 2.0):
            raise ValueError(f"`{name}` has to be a float in the [-2, 2] interval, but is {v}")
        out.append(float(x))
    if penalty_start is not None:
        if isinstance(penalty_start, bool) or not isinstance(penalty_start, int) or penalty_start < 0:
            raise ValueError(f"`penalty_start` has to be an integer >= 0, but is {penalty_start}")
    return out[0], out[1], penalty_start


DRY_KEYS = ("dry_multiplier", "dry_base", "dry_allowed_length", "dry_start", "dry_sequence_breakers")


def check_dry(dry_multiplier: Optional[float] = None, dry_base: Optional[float] = None, dry_allowed_length: Optional[int] = None,
              dry_start: Optional[int] = None, dry_sequence_breakers=None, vocab: Optional[int] = None):
    """the `dry_*` arguments of generate / sample -> (multiplier, base, allowed_length, start, breakers): multiplier 0.0 = off (None),
    base 1.75 and allowed_length 2 by default, start None = the caller's default (generate: the prompt length), breakers a tuple of at
    most 16 token ids (in [0, vocab) where the vocabulary is known).  Out of range: ValueError before anything runs"""
    def number(name, v, default, lo, hi):
        x = default if v is None else v
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not (lo <= x <= hi):      # (NaN fails the comparison)
            raise ValueError(f"`{name}` has to be a float in the [{lo}, {hi}] interval, but is {v}")
        return float(x)
    m = number("dry_multiplier", dry_multiplier, 0.0, 0.0, 100.0)
    b = number("dry_base", dry_base, 1.75, 1.0, 8.0)
    a = 2 if dry_allowed_length is None else dry_allowed_length
    if isinstance(a, bool) or not isinstance(a, int) or not (1 <= a <= _lib.DTK_DRY_MAX_MATCH):
        raise ValueError(f"`dry_allowed_length` has to be an integer in [1, {_lib.DTK_DRY_MAX_MATCH}], but is {dry_allowed_length}")
    if dry_start is not None:
        if isinstance(dry_start, bool) or not isinstance(dry_start, int) or dry_start < 0:
            raise ValueError(f"`dry_start` has to be an integer >= 0, but is {dry_start}")
    if isinstance(dry_sequence_breakers, (str, bytes)):
        raise ValueError("`dry_sequence_breakers` has to be a list of token ids, not a string")
    brk = tuple(dry_sequence_breakers) if dry_sequence_breakers is not None else ()
    if len(brk) > _lib.DTK_DRY_MAX_BREAKERS:
        raise ValueError(f"`dry_sequence_breakers` takes at most {_lib.DTK_DRY_MAX_BREAKERS} token ids, but has {len(brk)}")
    for t in brk:
        if isinstance(t, bool) or not isinstance(t, int) or t < 0 or (vocab is not None and t >= vocab):
            raise ValueError(f"`dry_sequence_breakers` has to hold token ids in [0, vocabulary), but holds {t!r}")
    return m, b, a, dry_start, brk


def dry_struct(multiplier: float, base: float, allowed_length: int, start: int, breakers=()) -> "_lib.DtkDry":
    d = _lib.DtkDry(float(multiplier), float(base), int(allowed_length), int(start), len(breakers))
    for i, t in enumerate(breakers):
        d.breakers[i] = int(t)
    return d


LENGTH_KEYS = ("min_new_tokens", "exponential_decay_length_penalty", "length_start")
SHAPE_KEYS = LENGTH_KEYS + ("logit_bias", "length_eos_ids")      # what a sequence's sampling dict carries of §3.1j


def check_length_control(min_new_tokens: Optional[int] = None, exponential_decay_length_penalty=None, length_start: Optional[int] = None):
    """the length arguments of generate / sample -> (min_new_tokens, decay, length_start): min_new_tokens 0 = off (None), decay None = off
    or (decay_start, factor) with factor finite and > 0, length_start None = the caller's default (generate: the prompt length).  A decay
    that starts below min_new_tokens is refused (HF would form -inf + inf there).  Out of range: ValueError before anything runs"""
    m = 0 if min_new_tokens is None else min_new_tokens
    if isinstance(m, bool) or not isinstance(m, int) or m < 0:
        raise ValueError(f"`min_new_tokens` has to be a positive integer, but is {min_new_tokens}")
    decay = None
    if exponential_decay_length_penalty is not None:
        d = exponential_decay_length_penalty
        if not isinstance(d, (tuple, list)) or len(d) != 2:
            raise ValueError(f"`exponential_decay_length_penalty` has to be a (start_index, decay_factor) pair, but is {d!r}")
        s, f = d
        if isinstance(s, bool) or not isinstance(s, int) or s < 0:
            raise ValueError(f"`exponential_decay_length_penalty`: start_index has to be an integer >= 0, but is {s!r}")
        if isinstance(f, bool) or not isinstance(f, (int, float)) or not (0.0 < f < math.inf):      # (NaN fails the comparison)
            raise ValueError(f"`exponential_decay_length_penalty`: decay_factor has to be a finite float > 0, but is {f!r}")
        if s < m:
            raise ValueError(f"`exponential_decay_length_penalty` starts at {s}, below `min_new_tokens` = {m}: the EOS logit would be "
                             f"-inf and decayed at once")
        decay = (int(s), float(f))      # (the double itself goes to the device: HF raises it, not its fp32 value, to the power k)
    if length_start is not None:
        if isinstance(length_start, bool) or not isinstance(length_start, int) or length_start < 0:
            raise ValueError(f"`length_start` has to be an integer >= 0, but is {length_start}")
    return int(m), decay, length_start


def check_logit_bias(logit_bias=None, sequence_bias=None, vocab: Optional[int] = None) -> Tuple[Tuple[int, float], ...]:
    """`logit_bias` ({id: value}, the OpenAI / vLLM argument) and HF's `sequence_bias` (dict with tuple keys, or list of [ids, value]) ->
    ((id, value), ...) in ascending id order without the entries whose value is 0.  Values finite in [-100, 100], at most DTK_BIAS_MAX ids
    in [0, vocab), every sequence of `sequence_bias` one token long (longer: NotImplementedError), no id in both (ValueError)"""
    out: Dict[int, float] = {}

    def put(name, t, v):
        if isinstance(t, str) and t.strip().lstrip("+").isdigit():      # (JSON object keys are strings)
            t = int(t)
        if isinstance(t, bool) or not isinstance(t, int) or t < 0 or (vocab is not None and t >= vocab):
            raise ValueError(f"`{name}` has to hold token ids in [0, vocabulary), but holds {t!r}")
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (-100.0 <= v <= 100.0):      # (NaN fails the comparison)
            raise ValueError(f"`{name}` has to hold finite biases in the [-100, 100] interval, but holds {v!r}")
        if t in out:
            raise ValueError(f"token id {t} is biased twice (`logit_bias` and `sequence_bias` are merged into one table)")
        out[t] = float(C.c_float(float(v)).value)

    if logit_bias is not None:
        if not isinstance(logit_bias, dict):
            raise ValueError(f"`logit_bias` has to be a dictionary {{token id: bias}}, but is {logit_bias!r}")
        for t, v in logit_bias.items():
            put("logit_bias", t, v)
    if sequence_bias is not None:
        if not isinstance(sequence_bias, (dict, list)) or len(sequence_bias) == 0:
            raise ValueError(f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {sequence_bias}.")
        items = list(sequence_bias.items()) if isinstance(sequence_bias, dict) else [tuple(e) if isinstance(e, (list, tuple)) else (e,) for e in sequence_bias]
        for e in items:
            if len(e) != 2 or not isinstance(e[0], (tuple, list)) or len(e[0]) == 0:
                raise ValueError(f"Each key in `sequence_bias` has to be a non-empty tuple of positive integers, but is {sequence_bias}.")
            if len(e[0]) > 1:
                raise NotImplementedError(f"sequence_bias: the multi-token sequence {tuple(e[0])} is not supported (single tokens only)")
            put("sequence_bias", e[0][0], e[1])
    pairs = tuple((t, out[t]) for t in sorted(out) if out[t] != 0.0)
    if len(pairs) > _lib.DTK_BIAS_MAX:
        raise ValueError(f"at most {_lib.DTK_BIAS_MAX} biased token ids, but {len(pairs)} are given")
    return pairs


def length_eos_ids(eos_ids, vocab: int) -> Tuple[int, ...]:
    """the EOS ids the length rules act on: the valid ones (an id outside the vocabulary, as -1, names none), ascending"""
    ids = tuple(sorted({int(t) for t in (eos_ids or ()) if 0 <= int(t) < vocab}))
    if len(ids) > _lib.DTK_LEN_MAX_EOS:
        raise ValueError(f"length control acts on at most {_lib.DTK_LEN_MAX_EOS} EOS ids, but {len(ids)} are given")
    return ids


def length_struct(min_new_tokens: int = 0, decay=None, start: int = 0, eos_ids=()) -> "_lib.DtkLengthCtl":
    s = _lib.DtkLengthCtl(int(min_new_tokens), int(decay[0]) if decay else 0, float(decay[1]) if decay else 0.0, int(start), len(eos_ids))
    for i, t in enumerate(eos_ids):
        s.eos_ids[i] = int(t)
    return s


def shape_of_sampling(sampling: Dict[str, Any], n_ids: int, vocab: Optional[int] = None):
    """a batch engine's view of a sequence's sampling dict -> (min_new_tokens, decay, length_start, eos ids, bias pairs), checked;
    length_start defaults to the sequence's prompt length, as penalty_start does"""
    m, decay, start = check_length_control(*(sampling.get(k) for k in LENGTH_KEYS))
    pairs = sampling.get("logit_bias") or ()
    pairs = check_logit_bias(dict(pairs) if not isinstance(pairs, dict) else pairs, None, vocab)
    eos = tuple(sampling.get("length_eos_ids") or ())
    on = bool(eos) and bool(m or decay)
    return (m if on else 0), (decay if on else None), ((n_ids if start is None else start) if on else 0), (eos if on else ()), pairs


def _is_neutral(value: Any, neutral: Any) -> bool:
    if neutral is None:
        return value is None
    if isinstance(neutral, (list, tuple)):          # "no extra processors"
        return isinstance(value, (list, tuple)) and len(value) == 0
    return isinstance(value, (bool, int, float)) and value == neutral


def _reject_unsupported_generate_kwargs(kw: Dict[str, Any]) -> None:
    for name, value in kw.items():
        allowed = _NEUTRAL_GENERATE_KWARGS.get(name)
        if allowed is None:
            raise TypeError(f"generate() got an argument this decoder does not implement: {name!r}")
        if allowed != "any" and not any(_is_neutral(value, a) for a in allowed):
            raise NotImplementedError(
                f"generate({name}={value!r}) is not supported: this path implements greedy / temperature / top-k / top-p / min-p / "
                f"epsilon-cutoff sampling of one sequence (the calls DetikzifyGenerator.generate makes); only {name} in {allowed} is accepted")


# forward() arguments of HF's LlamaForCausalLM / the reference's DetikzifyForConditionalGeneration that have no generate() twin, with
# the values at which forward(labels=...) computes what this path computes
_NEUTRAL_FORWARD_KWARGS: Dict[str, tuple] = {
    "return_dict": (None, True), "position_ids": (None,), "cache_position": (None,), "image_hidden_states": (None,),
    "pixel_attention_mask": (None,), "logits_to_keep": (None, 0), "num_logits_to_keep": (None, 0),
}
# the names of generate()'s table that HF's forward() has too: these pass generate()'s gate at its neutral values; every other name of
# that table (max_new_tokens' relatives, beams, penalties, streamers ...) is a TypeError here, as it is for HF's forward()
_FORWARD_SHARES_WITH_GENERATE = ("attention_mask", "use_cache", "past_key_values", "inputs_embeds", "output_attentions",
                                 "output_hidden_states", "output_logits")


def _reject_unsupported_forward_kwargs(kw: Dict[str, Any]) -> None:
    """the neutral-value gate of generate(), for forward(): names forward() does not have raise TypeError, known ones away from their
    neutral value NotImplementedError"""
    for name, value in kw.items():
        if name in _NEUTRAL_FORWARD_KWARGS:
            allowed = _NEUTRAL_FORWARD_KWARGS[name]
            if not any(_is_neutral(value, a) for a in allowed):
                raise NotImplementedError(f"forward({name}={value!r}) is not supported: only {name} in {allowed} is accepted")
        elif name in _FORWARD_SHARES_WITH_GENERATE:
            _reject_unsupported_generate_kwargs({name: value})
        else:
            raise TypeError(f"forward() got an argument this decoder does not implement: {name!r}")


def shifted_cross_entropy(logprobs: torch.Tensor, labels: torch.Tensor, first: int = 1, ignore_index: int = -100) -> torch.Tensor:
    """The loss of HF's causal LMs (reference v1/modeling_detikzify.py:260-271: logits[..., :-1, :] against labels[..., 1:] under
    CrossEntropyLoss()) from log-probabilities instead of logits: logprobs[k] = log p(ids[first + k] | ids[:first + k]) for the
    positions first .. T-1 of a sequence whose `labels` has T entries; a position counts iff its label is not `ignore_index` (a label
    that is kept equals the input id there: causal-LM labels are the ids with some positions masked).  Mean over the kept
    positions, float32 scalar; no kept position gives NaN (0 / 0), as torch's CrossEntropyLoss does.  Positions before `first` must
    all be ignored."""
    labels = torch.as_tensor(labels).reshape(-1)
    lp = torch.as_tensor(logprobs, dtype=torch.float32).reshape(-1)
    if lp.numel() != labels.numel() - first:
        raise ValueError(f"{lp.numel()} log-probabilities for labels[{first}:{labels.numel()}]")
    if bool((labels[1:first] != ignore_index).any()):
        raise ValueError("a label before `first` is not ignored: its log-probability was not computed")
    keep = labels[first:] != ignore_index
    # sum / count exactly as nll_loss(reduction="mean") reduces: float32 sum of the kept terms over their number
    return -(lp[keep].sum(dtype=torch.float32) / keep.sum().to(torch.float32))


class ScoreOutput(SimpleNamespace):
    """model.score()'s result: logprobs float32 [T - first], argmax int64 [T - first] (the greedy token at each scored position),
    lse float32 [T - first] (logsumexp of the position's logits), first (position of the first scored target)"""


class CausalLMLoss(SimpleNamespace):
    """CausalLMOutputWithPast stand-in of forward(labels=...): .loss (float32 scalar); .logits is never materialised (None).
    .logprobs / .first: the per-position log-probabilities the loss was reduced from"""


def _flat_ids(values) -> List[int]:
    """[id, [id, id], ...] -> flat list of ints (an eos_token_id may be a list in HF configs)"""
    out: List[int] = []
    for v in values or ():
        if isinstance(v, (list, tuple)):
            out.extend(int(x) for x in v)
        elif v is not None:
            out.append(int(v))
    return out


def rope_tables(c) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos/sin exactly as HF LlamaRotaryEmbedding computes them (modeling_llama.py:108-140): fp32 inv_freq (linear scaling:
    / factor; "llama3": modeling_rope_utils._compute_llama3_parameters), fp32 pos*inv_freq, cos/sin cast to bf16.  `c` has the
    DetikzifyConfig rope fields, head_dim and max_positions (a DetikzifyConfig or an AdapterConfig)."""
    inv = 1.0 / (c.rope_theta ** (torch.arange(0, c.head_dim, 2, dtype=torch.int64).float() / c.head_dim))
    if getattr(c, "rope_type", "linear") == "llama3":
        low_wl = c.rope_original_max_position / c.rope_low_freq_factor
        high_wl = c.rope_original_max_position / c.rope_high_freq_factor
        wavelen = 2 * math.pi / inv
        scaled = torch.where(wavelen > low_wl, inv / c.rope_factor, inv)
        smooth = (c.rope_original_max_position / wavelen - c.rope_low_freq_factor) / (c.rope_high_freq_factor - c.rope_low_freq_factor)
        mid = (1 - smooth) * scaled / c.rope_factor + smooth * scaled
        inv = torch.where((wavelen <= low_wl) & (wavelen >= high_wl), mid, scaled)
    elif c.rope_factor and c.rope_factor != 1.0:
        inv = inv / c.rope_factor
    freqs = torch.arange(c.max_positions, dtype=torch.float32)[:, None] * inv[None, :]
    return freqs.cos().to(torch.bfloat16), freqs.sin().to(torch.bfloat16)


def text_key(ids: torch.Tensor) -> int:
    """content hash of a text's token ids (the C side keys text-conditioned image prefixes by (image key, text key))"""
    b = ids.detach().to("cpu", torch.int64).reshape(-1).contiguous().numpy().tobytes()
    return int.from_bytes(hashlib.blake2b(b, digest_size=8).digest(), "little") or 1


DUMMY_IMAGE_KEY = 0x44554D4D59494D47     # image key of the adapter's dummy input (a text-only prompt)


def text_image_key(image_key: int, text_key_: int) -> int:
    """the key a text-conditioned slot's cache is stored under (dtk_text_image_key: the pair (image, text); 0 if either is 0)"""
    return int(_lib.load_library().dtk_text_image_key(C.c_uint64(int(image_key)), C.c_uint64(int(text_key_))))


def adapter_text(adapter_input_ids, adapter_attention_mask=None) -> torch.Tensor:
    """One prompt's text ids from the processor's adapter_input_ids / adapter_attention_mask.  One text has no padding; a
    mask with zeros (several differently padded texts batched together) is not implemented."""
    ids = torch.as_tensor(adapter_input_ids).detach().to("cpu", torch.int64)
    if ids.dim() == 2:
        if ids.shape[0] != 1:
            raise ValueError("batch size 1 only (one text per prompt)")
        ids = ids[0]
    if adapter_attention_mask is not None and not bool(torch.as_tensor(adapter_attention_mask).bool().all()):
        raise NotImplementedError("adapter_attention_mask with zeros (padded texts) is not supported: pass one unpadded text per prompt")
    if ids.numel() < 1:
        raise ValueError("empty adapter_input_ids")
    return ids.contiguous()


def _bf16_tensor_from_bits(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)


class DetikzifyForCausalLM:
    def __init__(self, config: DetikzifyConfig, device_index: int = 0):
        self.config = config
        self.lib = _lib.load_library()
        self.hip_device = int(device_index)
        kd = config.kernel_dict()
        cc = _lib.DtkConfig(**kd)
        cc.reserved[0] = int(getattr(config, "batch_slots", 0) or 0)
        cc.reserved[1] = {"fp8": 1, "mxfp4": 2}.get(getattr(config, "weight_format", "bf16"), 0)
        cc.reserved[2] = int(getattr(config, "kv_heads", 0) or 0)                       # GQA (v2)
        cc.reserved[3] = 0 if getattr(config, "proj_bias", True) else _lib.DTK_ARCH_PROJ_NO_BIAS
        cc.reserved[4] = {"bf16": 0, "mxfp8": 1}[getattr(config, "kv_format", "bf16")]   # key/value rows of decoded tokens
        ctx = C.c_void_p()
        rc = self.lib.dtk_create(C.byref(cc), self.hip_device, C.byref(ctx))
        if rc != 0:
            msg = self.lib.dtk_last_error(None)
            raise _lib.DtkError(f"dtk_create failed ({rc}): {msg.decode() if msg else ''} — "
                                "detikzify_amd needs an MI355X-class GPU; there is no CPU path")
        self._ctx = ctx
        self.generation_config = GenerationConfig(
            eos_token_id=config.eos_token_id, pad_token_id=config.pad_token_id,
            bos_token_id=config.bos_token_id)
        self.name_or_path = config.name_or_path
        self.model = SimpleNamespace(vision_model=DetikzifyVisionModel(self))
        self.reuse_prefix = False     # output-identical KV/image reuse across rollouts
        self.batch_engine = None      # set by infer.batching.BatchEngine: generate() then decodes in a slot
        # ViT passes (SelfSim reward) run on their own HIP stream and overlap with the decode steps of other sequences; they
        # share activation buffers with the image branch of a prefill, so those two are serialised by this lock (a reward
        # never takes the batch engine's lock: the trees that are decoding keep stepping)
        self._vit_lock = threading.RLock()
        self._single_busy = threading.Lock()     # held by a generate() that decodes on the context's single sequence
        self._weights_ready = False

    # ---- HF-shaped attributes ---------------------------------------------------------------
    @property
    def device(self) -> torch.device:
        # ids / pixels cross the C ABI as HOST buffers, so tensors handed to this model live on
        # the CPU; the GPU is self.hip_device.
        return torch.device("cpu")

    @property
    def dtype(self) -> torch.dtype:
        return torch.bfloat16

    def eval(self):
        return self

    def get_model(self):
        return self.model

    def __del__(self):
        try:
            if getattr(self, "_ctx", None):
                self.lib.dtk_destroy(self._ctx)
                self._ctx = None
        except Exception:
            pass

    def _check(self, rc, what):
        _lib.check(self.lib, self._ctx, rc, what)

    # ---- weights ------------------------------------------------------------------------------
    def tensor_names(self) -> List[str]:
        n = self.lib.dtk_num_tensors(self._ctx)
        return [self.lib.dtk_tensor_name(self._ctx, i).decode() for i in range(n)]

    def load_tensor(self, name: str, t: torch.Tensor):
        t = t.detach().cpu().contiguous()
        if t.dtype == torch.bfloat16:
            arr, dt = t.view(torch.int16).numpy(), _lib.DTK_BF16
        elif t.dtype == torch.float16:
            arr, dt = t.view(torch.int16).numpy(), _lib.DTK_F16
        else:
            arr, dt = t.float().numpy(), _lib.DTK_F32
        shape = (C.c_int64 * t.dim())(*t.shape) if t.dim() else (C.c_int64 * 1)(1)
        self._check(self.lib.dtk_load_tensor(self._ctx, name.encode(), arr.ctypes.data_as(C.c_void_p), dt,
                                             shape, max(t.dim(), 1)), f"dtk_load_tensor({name})")

    def load_state_dict(self, state: Dict[str, torch.Tensor], strict: bool = True):
        known = set(self.tensor_names())
        missing = sorted(k for k in known if k not in state and not k.startswith("rope."))
        unexpected = sorted(k for k in state if k not in known)
        if strict and (missing or unexpected):
            raise KeyError(f"missing: {missing[:5]}... unexpected: {unexpected[:5]}...")
        for k, v in state.items():
            if k in known:
                self.load_tensor(k, v)
        self._install_rope_tables()
        self._weights_ready = True
        return SimpleNamespace(missing_keys=missing, unexpected_keys=unexpected)

    def read_tensor(self, name: str) -> torch.Tensor:
        """stored bf16 tensor -> flat torch.bfloat16 (tests / CPU baseline)"""
        n = self.lib.dtk_tensor_numel(self._ctx, name.encode())
        if n < 0:
            raise KeyError(name)
        buf = np.empty(n, dtype=np.uint16)
        self._check(self.lib.dtk_read_tensor(self._ctx, name.encode(), buf.ctypes.data_as(C.c_void_p), n),
                    f"dtk_read_tensor({name})")
        return _bf16_tensor_from_bits(buf)

    def fill_synthetic(self, seed: int = 1234):
        self._check(self.lib.dtk_fill_synthetic(self._ctx, C.c_uint64(seed)), "dtk_fill_synthetic")
        self._install_rope_tables()
        self._weights_ready = True

    def _install_rope_tables(self):
        """cos/sin exactly as HF LlamaRotaryEmbedding computes them (modeling_llama.py:108-140):
        fp32 inv_freq (linear scaling: / factor; "llama3": modeling_rope_utils._compute_llama3_parameters),
        fp32 pos*inv_freq, cos/sin cast to bf16."""
        cos, sin = rope_tables(self.config)
        self.load_tensor("rope.cos", cos)
        self.load_tensor("rope.sin", sin)
        if self.has_adapter():
            cos, sin = rope_tables(self.adapter_config)
            self.load_tensor("embedding_model.rope.cos", cos)
            self.load_tensor("embedding_model.rope.sin", sin)

    # ---- TikZero adapter (text conditioning) ----------------------------------------------------------------------------
    def has_adapter(self) -> bool:
        return hasattr(self, "adapter")

    def create_adapter(self, acfg) -> None:
        """Register the adapter and its embedding model with the context (weights still to be loaded / filled)."""
        if self.config.arch == "v1":
            raise ValueError("Couldn't locate vision encoder layers! (the TikZero adapter needs a v2 checkpoint's SigLIP tower)")
        cc = _lib.DtkAdapterConfig(every_n=acfg.every_n, text_max=acfg.text_max, hidden=acfg.hidden, layers=acfg.layers,
                                   heads=acfg.heads, kv_heads=acfg.kv_heads, head_dim=acfg.head_dim, ffn=acfg.ffn, vocab=acfg.vocab,
                                   rms_eps=acfg.rms_eps, rope_theta=acfg.rope_theta, rope_factor=1.0,
                                   rope_low_freq_factor=acfg.rope_low_freq_factor, rope_high_freq_factor=acfg.rope_high_freq_factor,
                                   rope_original_max_position=acfg.rope_original_max_position)
        self._refuse_while_batch_busy("create_adapter")
        self._check(self.lib.dtk_adapter_create(self._ctx, C.byref(cc)), "dtk_adapter_create")
        self.adapter_epoch = getattr(self, "adapter_epoch", 0) + 1
        self.adapter_config = acfg
        self.adapter = SimpleNamespace(config=acfg)           # the reference's model.adapter / model.embedding_model attributes
        self.embedding_model = SimpleNamespace(config=acfg)

    def unload_cross_attn_adapter(self) -> None:
        """reference CrossAttentionAdapterMixin.unload_cross_attn_adapter: frees the adapter; image-only calls afterwards are those
        of a model that never had one"""
        if not self.has_adapter():
            raise AttributeError("no adapter is loaded")
        self._refuse_while_batch_busy("unload_cross_attn_adapter")
        with self._vit_lock:
            self._check(self.lib.dtk_adapter_destroy(self._ctx), "dtk_adapter_destroy")
        # every slot's cached ids are gone on the C side: a batch engine forgets which slot holds which prefix (it compares the epoch)
        self.adapter_epoch = getattr(self, "adapter_epoch", 0) + 1
        del self.adapter, self.embedding_model, self.adapter_config

    def _refuse_while_batch_busy(self, what: str) -> None:
        engine = getattr(self, "batch_engine", None)
        busy = getattr(engine, "busy", None)
        if callable(busy) and busy():
            raise _lib.DtkError(f"{what}() while sequences decode in the batch engine's slots: let them finish first")

    def embed_text(self, adapter_input_ids: torch.Tensor) -> torch.Tensor:
        """the embedding model's last_hidden_state [T, hidden] (bf16) of one text"""
        ids = adapter_text(adapter_input_ids)
        out = np.empty(ids.numel() * self.adapter_config.hidden, dtype=np.uint16)
        with self._vit_lock:
            self._check(self.lib.dtk_adapter_embed(self._ctx, ids.numpy().ctypes.data_as(C.c_void_p), ids.numel(),
                                                   out.ctypes.data_as(C.c_void_p)), "dtk_adapter_embed")
        return _bf16_tensor_from_bits(out).view(ids.numel(), self.adapter_config.hidden)

    # ---- vision tower -------------------------------------------------------------------------
    def vit_encode(self, pixel_values: Optional[torch.Tensor], want_pooled: bool = True, want_feats: bool = True,
                   adapter_input_ids: Optional[torch.Tensor] = None, adapter_attention_mask: Optional[torch.Tensor] = None):
        """(features, pooled); with adapter_input_ids the tower is conditioned on that text (pixel_values None: the adapter's
        dummy input, one image)"""
        if adapter_input_ids is not None:
            return self._vit_encode_text(pixel_values, want_pooled, want_feats, adapter_text(adapter_input_ids, adapter_attention_mask))
        if adapter_attention_mask is not None:
            raise ValueError("adapter_attention_mask without adapter_input_ids")
        px = pixel_values.detach().to("cpu", torch.float32).contiguous()
        if px.dim() == 3:
            px = px[None]
        B = px.shape[0]
        c = self.config
        n = (c.vit_image // c.vit_patch) ** 2
        feats = np.empty((B, n, c.vit_dim), dtype=np.uint16) if want_feats else None
        pooled = np.empty((B, c.vit_dim), dtype=np.uint16)
        with self._vit_lock:
            self._check(self.lib.dtk_vit_encode(
                self._ctx, px.numpy().ctypes.data_as(C.c_void_p), B, feats.ctypes.data_as(C.c_void_p) if want_feats else None,
                pooled.ctypes.data_as(C.c_void_p) if want_pooled else None), "dtk_vit_encode")
        f = _bf16_tensor_from_bits(feats.reshape(-1)).view(B, n, c.vit_dim) if want_feats else None
        p = _bf16_tensor_from_bits(pooled.reshape(-1)).view(B, c.vit_dim) if want_pooled else None
        return f, p

    def _vit_encode_text(self, pixel_values, want_pooled, want_feats, tids):
        if not self.has_adapter():
            raise TypeError("adapter_input_ids given but no adapter is loaded (load(..., adapter=True))")
        c = self.config
        px = None if pixel_values is None else pixel_values.detach().to("cpu", torch.float32).contiguous()
        if px is not None and px.dim() == 3:
            px = px[None]
        B = 1 if px is None else px.shape[0]
        n = (c.vit_image // c.vit_patch) ** 2
        feats = np.empty((B, n, c.vit_dim), dtype=np.uint16) if want_feats else None
        pooled = np.empty((B, c.vit_dim), dtype=np.uint16)
        with self._vit_lock:
            self._check(self.lib.dtk_vit_encode_text(
                self._ctx, None if px is None else px.numpy().ctypes.data_as(C.c_void_p), B, tids.numpy().ctypes.data_as(C.c_void_p),
                tids.numel(), C.c_uint64(text_key(tids)), feats.ctypes.data_as(C.c_void_p) if want_feats else None,
                pooled.ctypes.data_as(C.c_void_p) if want_pooled else None), "dtk_vit_encode_text")
        f = _bf16_tensor_from_bits(feats.reshape(-1)).view(B, n, c.vit_dim) if want_feats else None
        p = _bf16_tensor_from_bits(pooled.reshape(-1)).view(B, c.vit_dim) if want_pooled else None
        return f, p

    # ---- decoder ------------------------------------------------------------------------------
    def prefill(self, input_ids: torch.Tensor, pixel_values: Optional[torch.Tensor] = None,
                return_logits: bool = False, reuse: Optional[bool] = None, slot: Optional[int] = None,
                adapter_input_ids: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        if adapter_input_ids is not None:
            return self._prefill_text(input_ids, pixel_values, return_logits, reuse, slot, adapter_text(adapter_input_ids))
        ids = input_ids.detach().to("cpu", torch.int64).reshape(-1).contiguous()
        T = ids.numel()
        px_ptr, key = None, 0
        if pixel_values is not None:
            px = pixel_values.detach().to("cpu", torch.float32).contiguous()
            if px.dim() == 4:
                if px.shape[0] != 1:
                    raise ValueError("batch size 1 only")
                px = px[0]
            self._px_keepalive = px
            px_ptr = px.numpy().ctypes.data_as(C.c_void_p)
            key = self.image_key(pixel_values)
        reuse = self.reuse_prefix if reuse is None else reuse
        flags = (_lib.DTK_PREFILL_REUSE_PREFIX | _lib.DTK_PREFILL_REUSE_IMAGE) if reuse else 0
        logits = np.empty(self.config.vocab, dtype=np.float32) if return_logits else None
        lp = logits.ctypes.data_as(C.c_void_p) if return_logits else None
        with self._vit_lock:    # the image branch shares the ViT buffers with vit_encode (which runs on its own stream)
            if slot is None:
                self._check(self.lib.dtk_prefill(self._ctx, ids.numpy().ctypes.data_as(C.c_void_p), T, px_ptr,
                                                 C.c_uint64(key), flags, lp), "dtk_prefill")
            else:
                self._check(self.lib.dtk_prefill_slot(self._ctx, int(slot), ids.numpy().ctypes.data_as(C.c_void_p), T, px_ptr,
                                                      C.c_uint64(key), flags, lp), "dtk_prefill_slot")
        return torch.from_numpy(logits) if return_logits else None

    def _prefill_text(self, input_ids, pixel_values, return_logits, reuse, slot, tids):
        """prefill with the tower conditioned on one text (pixel_values None: the adapter's dummy input); the cached image prefix
        is keyed by (image, text)"""
        if not self.has_adapter():
            raise TypeError("adapter_input_ids given but no adapter is loaded (load(..., adapter=True))")
        ids = input_ids.detach().to("cpu", torch.int64).reshape(-1).contiguous()
        px_ptr, key = None, DUMMY_IMAGE_KEY
        if pixel_values is not None:
            px = pixel_values.detach().to("cpu", torch.float32).contiguous()
            if px.dim() == 4:
                if px.shape[0] != 1:
                    raise ValueError("batch size 1 only")
                px = px[0]
            self._px_keepalive = px
            px_ptr = px.numpy().ctypes.data_as(C.c_void_p)
            key = self.image_key(pixel_values)
        reuse = self.reuse_prefix if reuse is None else reuse
        flags = (_lib.DTK_PREFILL_REUSE_PREFIX | _lib.DTK_PREFILL_REUSE_IMAGE) if reuse else 0
        logits = np.empty(self.config.vocab, dtype=np.float32) if return_logits else None
        lp = logits.ctypes.data_as(C.c_void_p) if return_logits else None
        tp, tk = tids.numpy().ctypes.data_as(C.c_void_p), C.c_uint64(text_key(tids))
        with self._vit_lock:
            if slot is None:
                self._check(self.lib.dtk_prefill_text(self._ctx, ids.numpy().ctypes.data_as(C.c_void_p), ids.numel(), px_ptr,
                                                      C.c_uint64(key), tp, tids.numel(), tk, flags, lp), "dtk_prefill_text")
            else:
                self._check(self.lib.dtk_prefill_slot_text(self._ctx, int(slot), ids.numpy().ctypes.data_as(C.c_void_p), ids.numel(),
                                                           px_ptr, C.c_uint64(key), tp, tids.numel(), tk, flags, lp), "dtk_prefill_slot_text")
        return torch.from_numpy(logits) if return_logits else None

    # ---- scoring: teacher-forced log-probabilities of a given sequence in one pass ---------------------------------------------
    def default_first(self, ids: torch.Tensor) -> int:
        """the token after the last image token, or 1: the first position whose log-probability means something"""
        img = (ids == int(self.config.image_token_id)).nonzero()
        return max(1, int(img[-1]) + 1) if img.numel() else 1

    def score(self, input_ids: torch.Tensor, pixel_values: Optional[torch.Tensor] = None, first: Optional[int] = None,
              adapter_input_ids: Optional[torch.Tensor] = None, reuse: Optional[bool] = None,
              adapter_attention_mask: Optional[torch.Tensor] = None, top_logprobs: Optional[int] = None) -> ScoreOutput:
        """log p(ids[t] | ids[:t], image) for t = first .. T-1 in one prefill-sized pass (dtk_score): the lm_head runs over all
        scored rows with the log-softmax folded into its epilogue, no [T, V] logits exist.  Leaves the model as prefill() of the
        same arguments does (decode may continue).  first=None: the token after the last image token, or 1.  top_logprobs=k
        (1 .. 8): + .top_ids int64 / .top_logprobs float32, [T - first, k]: every scored position's k most likely tokens."""
        k = check_top_logprobs(top_logprobs)
        if not self._weights_ready:
            raise _lib.DtkError("no weights loaded (load_state_dict / fill_synthetic first)")
        self._refuse_while_batch_busy("score")
        ids = torch.as_tensor(input_ids).detach().to("cpu", torch.int64)
        if ids.dim() == 2:
            if ids.shape[0] != 1:
                raise ValueError("batch size 1 only")
            ids = ids[0]
        ids = ids.reshape(-1).contiguous()
        T = ids.numel()
        first = self.default_first(ids) if first is None else int(first)
        tids = None
        if adapter_input_ids is not None:
            if not self.has_adapter():
                raise TypeError("adapter_input_ids given but no adapter is loaded (load(..., adapter=True))")
            tids = adapter_text(adapter_input_ids, adapter_attention_mask)     # one unpadded text, as generate() takes it
        elif adapter_attention_mask is not None:
            raise ValueError("adapter_attention_mask without adapter_input_ids")
        px_ptr, key = None, (DUMMY_IMAGE_KEY if tids is not None else 0)
        if pixel_values is not None:
            px = pixel_values.detach().to("cpu", torch.float32).contiguous()
            if px.dim() == 4:
                if px.shape[0] != 1:
                    raise ValueError("batch size 1 only")
                px = px[0]
            self._px_keepalive = px
            px_ptr = px.numpy().ctypes.data_as(C.c_void_p)
            key = self.image_key(pixel_values)
        reuse = self.reuse_prefix if reuse is None else reuse
        flags = (_lib.DTK_PREFILL_REUSE_PREFIX | _lib.DTK_PREFILL_REUSE_IMAGE) if reuse else 0
        n = max(T - first, 1)
        lp, am, lse = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float32)
        outs = (int(first), lp.ctypes.data_as(C.c_void_p), am.ctypes.data_as(C.c_void_p), lse.ctypes.data_as(C.c_void_p))
        top_i, top_l = np.empty((n, k), dtype=np.int32), np.empty((n, k), dtype=np.float32)
        tops = (k, top_i.ctypes.data_as(C.c_void_p), top_l.ctypes.data_as(C.c_void_p))
        idp = ids.numpy().ctypes.data_as(C.c_void_p)
        if not self._single_busy.acquire(blocking=False):
            raise _lib.DtkError("score() while a generate() decodes on this model's single sequence")
        try:
            with self._vit_lock:
                if tids is None and k:
                    self._check(self.lib.dtk_score_top(self._ctx, idp, T, px_ptr, C.c_uint64(key), C.c_uint32(flags), *outs, *tops), "dtk_score_top")
                elif k:
                    self._check(self.lib.dtk_score_top_text(self._ctx, idp, T, px_ptr, C.c_uint64(key), tids.numpy().ctypes.data_as(C.c_void_p),
                                                            tids.numel(), C.c_uint64(text_key(tids)), C.c_uint32(flags), *outs, *tops),
                                "dtk_score_top_text")
                elif tids is None:
                    self._check(self.lib.dtk_score(self._ctx, idp, T, px_ptr, C.c_uint64(key), C.c_uint32(flags), *outs), "dtk_score")
                else:
                    self._check(self.lib.dtk_score_text(self._ctx, idp, T, px_ptr, C.c_uint64(key), tids.numpy().ctypes.data_as(C.c_void_p),
                                                        tids.numel(), C.c_uint64(text_key(tids)), C.c_uint32(flags), *outs), "dtk_score_text")
        finally:
            self._single_busy.release()
        return ScoreOutput(logprobs=torch.from_numpy(lp), argmax=torch.from_numpy(am).to(torch.int64), lse=torch.from_numpy(lse), first=first,
                           top_ids=torch.from_numpy(top_i).to(torch.int64) if k else None, top_logprobs=torch.from_numpy(top_l) if k else None)

    def score_candidates(self, prefix_ids: torch.Tensor, candidates: Sequence[Any], pixel_values: Optional[torch.Tensor] = None,
                         adapter_input_ids: Optional[torch.Tensor] = None, adapter_attention_mask: Optional[torch.Tensor] = None,
                         reuse: Optional[bool] = None, top_logprobs: Optional[int] = None) -> List[ScoreOutput]:
        """score(prefix + candidate, first=len(prefix)) for every candidate of one prompt, in input order, from ONE pass of the
        decoder over all candidates' rows (dtk_score_packed): the weights stream once, each candidate attends to the prompt and to
        itself.  Candidates that do not fit one pass (P - 1 + sum of lengths <= max_positions) are split by plan_packed_passes();
        the later passes reuse the prompt's cache.  Leaves the prompt's first P-1 positions cached and NO sequence to decode from:
        prefill() before decode_launch().  top_logprobs=k: as in score(), per candidate."""
        topk = check_top_logprobs(top_logprobs)
        if not self._weights_ready:
            raise _lib.DtkError("no weights loaded (load_state_dict / fill_synthetic first)")
        self._refuse_while_batch_busy("score_candidates")
        prefix = torch.as_tensor(prefix_ids).detach().to("cpu", torch.int64)
        if prefix.dim() == 2:
            if prefix.shape[0] != 1:
                raise ValueError("batch size 1 only")
            prefix = prefix[0]
        prefix = prefix.reshape(-1).contiguous()
        P = prefix.numel()
        cands = [torch.as_tensor(c).detach().to("cpu", torch.int64).reshape(-1).contiguous() for c in candidates]
        if not cands:
            raise ValueError("score_candidates: no candidates")
        lens = [c.numel() for c in cands]
        passes = plan_packed_passes(P, lens, int(self.config.max_positions))
        tids = None
        if adapter_input_ids is not None:
            if not self.has_adapter():
                raise TypeError("adapter_input_ids given but no adapter is loaded (load(..., adapter=True))")
            tids = adapter_text(adapter_input_ids, adapter_attention_mask)
        elif adapter_attention_mask is not None:
            raise ValueError("adapter_attention_mask without adapter_input_ids")
        px_ptr, key = None, (DUMMY_IMAGE_KEY if tids is not None else 0)
        if pixel_values is not None:
            px = pixel_values.detach().to("cpu", torch.float32).contiguous()
            if px.dim() == 4:
                if px.shape[0] != 1:
                    raise ValueError("batch size 1 only")
                px = px[0]
            self._px_keepalive = px
            px_ptr = px.numpy().ctypes.data_as(C.c_void_p)
            key = self.image_key(pixel_values)
        reuse = self.reuse_prefix if reuse is None else reuse
        reuse_flags = _lib.DTK_PREFILL_REUSE_PREFIX | _lib.DTK_PREFILL_REUSE_IMAGE
        pfx = prefix.numpy().ctypes.data_as(C.c_void_p)
        out: List[ScoreOutput] = []
        if not self._single_busy.acquire(blocking=False):
            raise _lib.DtkError("score_candidates() while a generate() decodes on this model's single sequence")
        try:
            for k, members in enumerate(passes):
                ids = torch.cat([cands[i] for i in members]).contiguous()
                clen = np.asarray([lens[i] for i in members], dtype=np.int32)
                n = ids.numel()
                lp, am, lse = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float32)
                flags = reuse_flags if (reuse or k > 0) else 0       # a later pass always continues the first one's prompt
                tail = (ids.numpy().ctypes.data_as(C.c_void_p), clen.ctypes.data_as(C.c_void_p), len(members),
                        lp.ctypes.data_as(C.c_void_p), am.ctypes.data_as(C.c_void_p), lse.ctypes.data_as(C.c_void_p))
                top_i, top_l = np.empty((n, topk), dtype=np.int32), np.empty((n, topk), dtype=np.float32)
                tops = (topk, top_i.ctypes.data_as(C.c_void_p), top_l.ctypes.data_as(C.c_void_p))
                with self._vit_lock:
                    if tids is None and topk:
                        self._check(self.lib.dtk_score_packed_top(self._ctx, pfx, P, px_ptr, C.c_uint64(key), C.c_uint32(flags), *tail, *tops),
                                    "dtk_score_packed_top")
                    elif topk:
                        self._check(self.lib.dtk_score_packed_top_text(self._ctx, pfx, P, px_ptr, C.c_uint64(key),
                                                                       tids.numpy().ctypes.data_as(C.c_void_p), tids.numel(),
                                                                       C.c_uint64(text_key(tids)), C.c_uint32(flags), *tail, *tops),
                                    "dtk_score_packed_top_text")
                    elif tids is None:
                        self._check(self.lib.dtk_score_packed(self._ctx, pfx, P, px_ptr, C.c_uint64(key), C.c_uint32(flags), *tail),
                                    "dtk_score_packed")
                    else:
                        self._check(self.lib.dtk_score_packed_text(self._ctx, pfx, P, px_ptr, C.c_uint64(key),
                                                                   tids.numpy().ctypes.data_as(C.c_void_p), tids.numel(),
                                                                   C.c_uint64(text_key(tids)), C.c_uint32(flags), *tail), "dtk_score_packed_text")
                lo = 0
                for i in members:
                    hi = lo + lens[i]
                    out.append(ScoreOutput(logprobs=torch.from_numpy(lp[lo:hi].copy()), argmax=torch.from_numpy(am[lo:hi]).to(torch.int64),
                                           lse=torch.from_numpy(lse[lo:hi].copy()), first=P,
                                           top_ids=torch.from_numpy(top_i[lo:hi]).to(torch.int64) if topk else None,
                                           top_logprobs=torch.from_numpy(top_l[lo:hi].copy()) if topk else None))
                    lo = hi
        finally:
            self._single_busy.release()
        return out

    def forward(self, input_ids: Optional[torch.Tensor] = None, pixel_values: Optional[torch.Tensor] = None,
                labels: Optional[torch.Tensor] = None, adapter_input_ids: Optional[torch.Tensor] = None, **hf_kwargs) -> CausalLMLoss:
        """model(input_ids=..., pixel_values=..., labels=...).loss of the reference's causal LM (shift by one, CrossEntropyLoss():
        mean over the positions whose label is not -100), reduced on the host from the device's log-probabilities.  Logits of
        every position are never materialised: labels=None or output_logits=True raise."""
        if hf_kwargs.get("output_logits"):
            raise NotImplementedError("forward(output_logits=True): the [T, V] logits are never materialised; "
                                      "model.prefill(ids, pixel_values, return_logits=True) returns one row")
        tmask = hf_kwargs.pop("adapter_attention_mask", None)
        _reject_unsupported_forward_kwargs(hf_kwargs)
        if labels is None:
            raise NotImplementedError("forward() without labels would return the logits of every position, which are never materialised: "
                                      "pass labels for the loss, model.score() for log-probabilities, or "
                                      "model.prefill(ids, pixel_values, return_logits=True) for one row of logits")
        if input_ids is None:
            raise ValueError("forward() needs input_ids")
        ids = torch.as_tensor(input_ids).detach().to("cpu", torch.int64)
        lab = torch.as_tensor(labels).detach().to("cpu", torch.int64)
        if ids.dim() == 2:
            if ids.shape[0] != 1:
                raise ValueError("batch size 1 only")
            ids = ids[0]
        lab = lab.reshape(-1)
        if lab.numel() != ids.numel():
            raise ValueError(f"labels of {lab.numel()} entries for {ids.numel()} input ids")
        kept = (lab != -100).nonzero().reshape(-1)
        kept = kept[kept >= 1]                      # label 0 has no context: the shift drops it
        if bool((lab[kept] != ids[kept]).any()):
            raise NotImplementedError("labels that differ from input_ids at a position that is not -100")
        if kept.numel() == 0:
            return CausalLMLoss(loss=torch.tensor(float("nan"), dtype=torch.float32), logits=None, logprobs=torch.empty(0), first=ids.numel())
        first = int(kept[0])
        out = self.score(ids, pixel_values, first=first, adapter_input_ids=adapter_input_ids, adapter_attention_mask=tmask)
        return CausalLMLoss(loss=shifted_cross_entropy(out.logprobs, lab, first=first), logits=None, logprobs=out.logprobs, first=first)

    __call__ = forward

    def set_sampling(self, do_sample=False, temperature=1.0, top_p=1.0, top_k=0, seed=0,
                     bad_ids: Iterable[int] = (), begin_suppress_ids: Iterable[int] = (),
                     always_suppress_ids: Iterable[int] = (), slot: Optional[int] = None, min_p: float = 0.0,
                     epsilon_cutoff: float = 0.0):
        """the sampling configuration of the single sequence (slot None) or of a slot.  min_p / epsilon_cutoff (HF's two warpers behind
        top-p; 0 = off) travel in a call of their own, set_sampling_ext: the plain call resets both."""
        min_p, epsilon_cutoff = check_truncation(min_p, epsilon_cutoff)
        s = _lib.DtkSampling()
        s.do_sample, s.temperature, s.top_p, s.top_k = int(bool(do_sample)), float(temperature), float(top_p), int(top_k or 0)
        s.seed = int(seed) & ((1 << 64) - 1)
        for field, cnt, vals in (("bad_ids", "n_bad", bad_ids), ("begin_suppress_ids", "n_begin_suppress", begin_suppress_ids),
                                 ("always_suppress_ids", "n_always_suppress", always_suppress_ids)):
            vals = [int(v) for v in vals]
            if len(vals) > 8:
                raise ValueError("at most 8 ids per suppression list")
            setattr(s, cnt, len(vals))
            arr = getattr(s, field)
            for i, v in enumerate(vals):
                arr[i] = v
        if slot is None:
            self._check(self.lib.dtk_set_sampling(self._ctx, C.byref(s)), "dtk_set_sampling")
        else:
            self._check(self.lib.dtk_set_sampling_slot(self._ctx, int(slot), C.byref(s)), "dtk_set_sampling_slot")
        if min_p or epsilon_cutoff:
            self.set_sampling_ext(min_p, epsilon_cutoff, slot=slot)

    def set_sampling_ext(self, min_p: float = 0.0, epsilon_cutoff: float = 0.0, slot: Optional[int] = None):
        """min_p / epsilon_cutoff of the configuration the last set_sampling left (dtk_set_sampling_ext / dtk_set_sampling_slot_ext);
        set_sampling itself resets both to 0"""
        min_p, epsilon_cutoff = check_truncation(min_p, epsilon_cutoff)
        fn = getattr(self.lib, "dtk_set_sampling_ext" if slot is None else "dtk_set_sampling_slot_ext", None)
        if fn is None:          # a device without the two calls has nothing to reset
            if min_p or epsilon_cutoff:
                raise _lib.DtkError("this device takes no min_p / epsilon_cutoff")
            return
        x = _lib.DtkSamplingExt(min_p=min_p, epsilon_cutoff=epsilon_cutoff)
        if slot is None:
            self._check(fn(self._ctx, C.byref(x)), "dtk_set_sampling_ext")
        else:
            self._check(fn(self._ctx, int(slot), C.byref(x)), "dtk_set_sampling_slot_ext")

    def set_penalties(self, presence: float = 0.0, frequency: float = 0.0, start: int = 0, slot: Optional[int] = None):
        """presence / frequency penalty of the sequence the last set_sampling configured (dtk_set_penalties / dtk_set_penalties_slot):
        z'[i] = z[i] - (presence + frequency * count[i]) for every id counted among the sequence's tokens from position `start` on
        (DESIGN §3.1h).  set_sampling itself resets the three values to 0"""
        presence, frequency, start = check_penalties(presence, frequency, int(start))
        fn = getattr(self.lib, "dtk_set_penalties" if slot is None else "dtk_set_penalties_slot", None)
        if fn is None:          # a device without the two calls has nothing to reset
            if presence or frequency:
                raise _lib.DtkError("this device takes no presence / frequency penalty")
            return
        if slot is None:
            self._check(fn(self._ctx, presence, frequency, start), "dtk_set_penalties")
        else:
            self._check(fn(self._ctx, int(slot), presence, frequency, start), "dtk_set_penalties_slot")

    def set_dry(self, multiplier: float = 0.0, base: float = 1.75, allowed_length: int = 2, start: int = 0, breakers=(),
                slot: Optional[int] = None):
        """DRY of the sequence the last set_sampling configured (dtk_set_dry / dtk_set_dry_slot): the token that would extend a verbatim
        repetition of length M >= allowed_length of the sequence's own text from position `start` on has multiplier * base^(M -
        allowed_length) taken off its logit.  set_sampling itself resets it to off"""
        m, b, a, st, brk = check_dry(multiplier, base, allowed_length, int(start), breakers, int(self.config.vocab))
        fn = getattr(self.lib, "dtk_set_dry" if slot is None else "dtk_set_dry_slot", None)
        if fn is None:          # a device without the two calls has nothing to reset
            if m:
                raise _lib.DtkError("this device takes no DRY penalty")
            return
        d = dry_struct(m, b, a, st, brk)
        if slot is None:
            self._check(fn(self._ctx, C.byref(d)), "dtk_set_dry")
        else:
            self._check(fn(self._ctx, int(slot), C.byref(d)), "dtk_set_dry_slot")

    def dry_history(self, slot: Optional[int] = None) -> torch.Tensor:
        """diagnostic: the token history the sequence's next DRY scan will read (empty while DRY is off)"""
        cap = int(self.lib.dtk_max_positions(self._ctx))
        out = (C.c_int32 * cap)()
        n = int(self.lib.dtk_dry_history(self._ctx, -1 if slot is None else int(slot), out, cap))
        if n < 0:
            self._check(n, "dtk_dry_history")
        return torch.tensor(list(out[:n]), dtype=torch.int64)

    def set_length_control(self, min_new_tokens: int = 0, decay=None, start: int = 0, eos_ids=(), slot: Optional[int] = None):
        """the length rules of the sequence the last set_sampling configured (dtk_set_length_control[_slot]): with n = the sequence's
        length - `start`, the logits of `eos_ids` are -inf while n < min_new_tokens and grow by |z| * (factor^(n - decay_start) - 1)
        once n > decay_start, decay = (decay_start, factor).  set_sampling itself resets them to off"""
        m, decay, st = check_length_control(min_new_tokens, decay, int(start))
        eos = length_eos_ids(eos_ids, int(self.config.vocab))
        on = bool(eos) and bool(m or decay)
        fn = getattr(self.lib, "dtk_set_length_control" if slot is None else "dtk_set_length_control_slot", None)
        if fn is None:          # a device without the two calls has nothing to reset
            if on:
                raise _lib.DtkError("this device takes no length control")
            return
        s = length_struct(m, decay, st, eos)
        if slot is None:
            self._check(fn(self._ctx, C.byref(s)), "dtk_set_length_control")
        else:
            self._check(fn(self._ctx, int(slot), C.byref(s)), "dtk_set_length_control_slot")

    def set_logit_bias(self, logit_bias=None, slot: Optional[int] = None):
        """the bias table of the sequence the last set_sampling configured (dtk_set_logit_bias[_slot]): {id: value} or (id, value) pairs,
        at most 256, added to the raw logits in front of everything else.  None / empty clears; set_sampling itself does"""
        pairs = check_logit_bias(dict(logit_bias or ()), None, int(self.config.vocab))
        fn = getattr(self.lib, "dtk_set_logit_bias" if slot is None else "dtk_set_logit_bias_slot", None)
        if fn is None:          # a device without the two calls has nothing to reset
            if pairs:
                raise _lib.DtkError("this device takes no logit bias")
            return
        n = len(pairs)
        ids = (C.c_int32 * max(n, 1))(*[t for t, _ in pairs])
        vals = (C.c_float * max(n, 1))(*[v for _, v in pairs])
        if slot is None:
            self._check(fn(self._ctx, ids, vals, n), "dtk_set_logit_bias")
        else:
            self._check(fn(self._ctx, int(slot), ids, vals, n), "dtk_set_logit_bias_slot")

    def logit_bias_table(self, slot: Optional[int] = None) -> torch.Tensor:
        """diagnostic: the dense bias table the sequence's next sampler will read (float32 per vocabulary entry; zeros while off)"""
        V = int(self.config.vocab)
        out = np.zeros(V, dtype=np.float32)
        n = int(self.lib.dtk_logit_bias_table(self._ctx, -1 if slot is None else int(slot), out.ctypes.data_as(C.POINTER(C.c_float)), V))
        if n < 0:
            self._check(n, "dtk_logit_bias_table")
        return torch.from_numpy(out)

    def token_counts(self, slot: Optional[int] = None) -> torch.Tensor:
        """diagnostic: the count table the sequence's next step will read (uint16 per vocabulary entry, as int32)"""
        V = int(self.config.vocab)
        out = (C.c_uint16 * V)()
        self._check(self.lib.dtk_token_counts(self._ctx, -1 if slot is None else int(slot), out, V), "dtk_token_counts")
        return torch.tensor(list(out), dtype=torch.int32)

    # ---- batched decode (independent rollouts share one pass over the weights) -----------------------
    def num_slots(self) -> int:
        return int(self.lib.dtk_num_slots(self._ctx))

    def max_decode_slots(self) -> int:
        """slots 0..n-1 that may take part in a decode step: 4 (contexts with <= 5 slots: multi-vector kernels), 16, 32 or 64
        (one, two, four MFMA column tiles), never more than num_slots()"""
        return int(self.lib.dtk_max_decode_slots(self._ctx))

    def decode_batch_launch(self, active_slots: Iterable[int]):
        arr = (C.c_int32 * _lib.DTK_MAX_BATCH)()
        for j in active_slots:
            arr[int(j)] = 1
        self._check(self.lib.dtk_decode_batch_launch(self._ctx, arr), "dtk_decode_batch_launch")

    def decode_batch_wait(self, top: bool = False):
        """every slot's token of the oldest unread step (-1: took no part).  top=True (needs enable_top_logprobs(k)): (tokens, logprobs,
        sample_logprobs, top_ids, top_logprobs), the last two one list of k entries per slot ((-1, NaN) entries where there is no token)"""
        out = (C.c_int64 * _lib.DTK_MAX_BATCH)()
        if top:
            lp, slp = (C.c_float * _lib.DTK_MAX_BATCH)(), (C.c_float * _lib.DTK_MAX_BATCH)()
            n, k = _lib.DTK_MAX_BATCH * _lib.DTK_MAX_TOP, self.top_logprobs_enabled
            ti, tl = (C.c_int32 * n)(), (C.c_float * n)()
            self._check(self.lib.dtk_decode_batch_wait_top(self._ctx, out, lp, slp, ti, tl), "dtk_decode_batch_wait_top")
            rows = [slice(j * _lib.DTK_MAX_TOP, j * _lib.DTK_MAX_TOP + k) for j in range(_lib.DTK_MAX_BATCH)]
            return [int(v) for v in out], list(lp), list(slp), [list(ti[r]) for r in rows], [list(tl[r]) for r in rows]
        self._check(self.lib.dtk_decode_batch_wait(self._ctx, out), "dtk_decode_batch_wait")
        return [int(v) for v in out]

    def decode_batch_wait_lp(self) -> Tuple[List[int], List[float], List[float]]:
        """decode_batch_wait + every slot's (logprob, sample_logprob); needs enable_logprobs()"""
        out = (C.c_int64 * _lib.DTK_MAX_BATCH)()
        lp, slp = (C.c_float * _lib.DTK_MAX_BATCH)(), (C.c_float * _lib.DTK_MAX_BATCH)()
        self._check(self.lib.dtk_decode_batch_wait_lp(self._ctx, out, lp, slp), "dtk_decode_batch_wait_lp")
        return [int(v) for v in out], list(lp), list(slp)

    # ---- prompt-lookup speculative decoding of slot 0 (dtk_spec_*) ------------------------------
    def spec_begin(self, num_tokens: int, max_ngram: int = 2, table: bool = False) -> None:
        """slot 0 (prefilled, logits pending) decodes up to num_tokens + 1 tokens per step from here to spec_end(): the step's vectors
        are consecutive positions of the one sequence.  table=True: the drafts come from spec_set_drafts (tests) instead of the lookup"""
        self._check(self.lib.dtk_spec_begin(self._ctx, int(num_tokens), int(max_ngram),
                                            _lib.DTK_SPEC_TABLE if table else _lib.DTK_SPEC_LOOKUP), "dtk_spec_begin")

    def spec_set_drafts(self, table: Sequence[int]) -> None:
        """the draft of every absolute position (-1 = none) for spec_begin(table=True)"""
        arr = (C.c_int32 * max(1, len(table)))(*[int(v) for v in table])
        self._check(self.lib.dtk_spec_set_drafts(self._ctx, arr, len(table)), "dtk_spec_set_drafts")

    def spec_launch(self) -> None:
        self._check(self.lib.dtk_spec_launch(self._ctx), "dtk_spec_launch")

    def spec_wait(self, logprobs: bool = False):
        """the tokens the oldest unread speculative step accepted (1 .. num_tokens + 1); logprobs=True: (tokens, logprobs,
        sample_logprobs)"""
        out, n = (C.c_int64 * 4)(), C.c_int(0)
        lp, slp = ((C.c_float * 4)(), (C.c_float * 4)()) if logprobs else (None, None)
        self._check(self.lib.dtk_spec_wait(self._ctx, out, C.byref(n), lp, slp), "dtk_spec_wait")
        toks = [int(out[i]) for i in range(n.value)]
        return (toks, [float(lp[i]) for i in range(n.value)], [float(slp[i]) for i in range(n.value)]) if logprobs else toks

    def spec_end(self, keep_len: int) -> None:
        """end the speculation: slot 0 keeps its first keep_len ids and has no pending logits (the next prefill recomputes one row)"""
        self._check(self.lib.dtk_spec_end(self._ctx, int(keep_len)), "dtk_spec_end")

    def op_spec_lookup(self, ids: Sequence[int], num_tokens: int, max_ngram: int = 2, max_positions: Optional[int] = None) -> List[int]:
        """the lookup kernel alone over ids: the drafts a step whose vector 0 forwards ids[-1] would carry"""
        n = len(ids)
        arr = (C.c_int32 * max(1, n))(*[int(v) for v in ids])
        out, k = (C.c_int32 * 4)(), C.c_int(0)
        self._check(self.lib.dtk_op_spec_lookup(self._ctx, arr, n, int(num_tokens), int(max_ngram),
                                                int(max(n, 1) + 8 if max_positions is None else max_positions), out, C.byref(k)),
                    "dtk_op_spec_lookup")
        return [int(out[i]) for i in range(k.value)]

    def spec_set_corpus(self, seqs) -> int:
        """the lookup's second draft source: 1-D id sequences (earlier programs, boilerplate), joined by a -1 separator into one corpus of
        at most DTK_SPEC_CORPUS_MAX entries; empty sequences are dropped, no sequence clears it.  Returns the entries set.  It stays
        until it is cleared (generate(prompt_lookup_corpus=) sets it for one call)"""
        flat = flatten_corpus(seqs, int(self.config.vocab))
        self._spec_set_corpus(flat)
        return len(flat)

    def _spec_set_corpus(self, flat: Sequence[int]) -> None:
        """the flat corpus as flatten_corpus makes it (generate() has checked it already); [] clears"""
        arr = (C.c_int32 * max(1, len(flat)))(*flat)
        self._check(_lib.corpus_call(self.lib, "dtk_spec_set_corpus")(self._ctx, arr, len(flat)), "dtk_spec_set_corpus")

    def spec_corpus_len(self) -> int:
        return int(_lib.corpus_call(self.lib, "dtk_spec_corpus_len")(self._ctx))

    def spec_counters(self) -> Tuple[int, int, int]:
        """(history, corpus, none): the steps launched since spec_begin whose drafts came from there"""
        out = (C.c_int64 * 3)()
        self._check(_lib.corpus_call(self.lib, "dtk_spec_counters")(self._ctx, out), "dtk_spec_counters")
        return int(out[0]), int(out[1]), int(out[2])

    def spec_lookup_corpus(self, ids: Sequence[int], corpus: Sequence[int], num_tokens: int, max_ngram: int = 2,
                           max_positions: Optional[int] = None) -> Tuple[List[int], int, int]:
        """the two lookup kernels alone over ids and a flat corpus (negative entries separate its sequences): (drafts, source, n) — the
        drafts a step whose vector 0 forwards ids[-1] would carry, where they came from (DTK_SPEC_FROM_*) and the n-gram size that matched"""
        n, nc = len(ids), len(corpus)
        arr = (C.c_int32 * max(1, n))(*[int(v) for v in ids])
        carr = (C.c_int32 * max(1, nc))(*[int(v) for v in corpus])
        out, k, src, ng = (C.c_int32 * 4)(), C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(_lib.corpus_call(self.lib, "dtk_op_spec_lookup_corpus")(
            self._ctx, arr, n, carr, nc, int(num_tokens), int(max_ngram), int(max(n, 1) + 8 if max_positions is None else max_positions),
            out, C.byref(k), C.byref(src), C.byref(ng)), "dtk_op_spec_lookup_corpus")
        return [int(out[i]) for i in range(k.value)], int(src.value), int(ng.value)

    # ---- classifier-free guidance: pairs of batch slots (dtk_set_guidance) ------------------------------------
    def set_guidance(self, scale: Optional[float], cond_slot: int, uncond_slot: Optional[int]):
        """pairs two decoding slots for classifier-free guidance: in every batched step the conditional slot's pending
        logits row becomes scale * (log_softmax(zc) - log_softmax(zu)) + log_softmax(zu) in front of its whole sampler chain, and the
        unconditional slot forwards the token that chain chose.  scale None / 1 or uncond_slot None / < 0 dissolves the pair cond_slot
        heads.  Refused while a batch step is in flight"""
        g = check_guidance_scale(scale)
        u = -1 if uncond_slot is None else int(uncond_slot)
        self._check(self.lib.dtk_set_guidance(self._ctx, int(cond_slot), u, g), "dtk_set_guidance")

    def reserve_guidance(self, n_pairs: int) -> None:
        """standing pairs (dtk_reserve_guidance): the captured batched steps are shaped for n_pairs guided pairs from here on, so forming
        or dissolving a pair or changing its scale only writes the device's pair table and re-captures nothing; a live pair computes what
        it computes without a reservation, bit for bit.  0 ends the reservation.  Refused while a batch step is in flight"""
        self._check(self.lib.dtk_reserve_guidance(self._ctx, int(n_pairs)), "dtk_reserve_guidance")

    @property
    def batch_graph_captures(self) -> int:
        """captures of a batched decode step since the context was created (a re-capture shows as an increment)"""
        return int(self.lib.dtk_batch_graph_captures(self._ctx))

    def guidance(self, slot: int) -> Optional[Dict[str, Any]]:
        """diagnostic: the guided pair `slot` is in — {partner, is_cond, scale, lse: (Lc, Lu) of the pair's last step} — or None"""
        partner, is_cond, scale, lse = C.c_int(-1), C.c_int(0), C.c_float(1.0), (C.c_float * 2)()
        self._check(self.lib.dtk_get_guidance(self._ctx, int(slot), C.byref(partner), C.byref(is_cond), C.byref(scale), lse), "dtk_get_guidance")
        if partner.value < 0:
            return None
        return dict(partner=int(partner.value), is_cond=bool(is_cond.value), scale=float(scale.value), lse=(float(lse[0]), float(lse[1])))

    # ---- log-probabilities of sampled tokens (dtk_set_option "logprobs") ------------------------------------
    @property
    def logprobs_enabled(self) -> bool:
        return bool(getattr(self, "_logprobs", False))

    def enable_logprobs(self) -> None:
        """every decode step from here on also delivers its token's (logprob, sample_logprob); stays on.  Refused while a batch step
        is in flight, single-sequence steps are unread or an engine holds a sequence: a batch engine switches it on before its first join"""
        if not self.logprobs_enabled:
            self.set_option("logprobs", 1)
            self._logprobs = True

    def disable_logprobs(self) -> None:
        """the steps stop delivering the pairs (refused where enable_logprobs() is, and while top_logprobs_enabled): what a batch engine
        built with top_logprobs= does on close() for a model it found without them"""
        if self.logprobs_enabled:
            self.set_option("logprobs", 0)
            self._logprobs = False

    @property
    def top_logprobs_enabled(self) -> int:
        return int(getattr(self, "_top_logprobs", 0))

    def enable_top_logprobs(self, k: int) -> None:
        """every decode step from here on also leaves the k (1 .. 8; 0: none again) most likely tokens of the logits it sampled from:
        decode_wait(top=True) / decode_batch_wait(top=True).  Switches the log-probabilities on if needed; refused where they are."""
        k = int(k)
        if not 0 <= k <= _lib.DTK_MAX_TOP:
            raise ValueError(f"top_logprobs = {k}: 0 .. {_lib.DTK_MAX_TOP}")
        if k:
            self.enable_logprobs()
        if k != self.top_logprobs_enabled:
            self.set_option("top_logprobs", k)
            self._top_logprobs = k

    def kv_fork(self, src_slot: int, dst_slot: int, n_tokens: int):
        self._check(self.lib.dtk_kv_fork(self._ctx, int(src_slot), int(dst_slot), int(n_tokens)), "dtk_kv_fork")

    _image_keys: Dict[Tuple[int, int, int], Tuple[Any, int]] = {}     # (storage address, elements, tensor version) -> (tensor, key)
    _image_keys_lock = threading.Lock()     # every tree thread of a parallel search comes through image_key()

    @classmethod
    def image_key(cls, pixel_values: torch.Tensor) -> int:
        """content hash of the pixels (the C side keys cached image prefixes by it).  Hashing 1.8 MB costs ~2 ms under the GIL and
        the 64 trees of a parallel search all present the SAME tensor object: memoised per tensor (the entry keeps the tensor
        alive, so its address cannot be reused by another one; the version counter catches in-place edits)"""
        # (inference-mode tensors keep no version counter: an in-place edit of one between two calls would go unnoticed —
        # processor outputs are never edited)
        ident = (pixel_values.data_ptr(), pixel_values.numel(), -1 if pixel_values.is_inference() else pixel_values._version)
        with cls._image_keys_lock:
            hit = cls._image_keys.get(ident)
        if hit is not None and hit[0] is pixel_values:
            return hit[1]
        px = pixel_values.detach().to("cpu", torch.float32).contiguous()
        key = int.from_bytes(hashlib.blake2b(px.numpy().tobytes(), digest_size=8).digest(), "little")    # (outside the lock: 2 ms)
        with cls._image_keys_lock:
            while len(cls._image_keys) >= 64:       # oldest entry out (dicts keep insertion order); at most 64 pixel tensors stay alive
                cls._image_keys.pop(next(iter(cls._image_keys)))
            cls._image_keys[ident] = (pixel_values, key)
        return key

    def slot_lcp(self, slot: int, ids: torch.Tensor, key: int = 0) -> int:
        ids = ids.detach().to("cpu", torch.int64).reshape(-1).contiguous()
        out = C.c_int(0)
        self._check(self.lib.dtk_slot_lcp(self._ctx, int(slot), ids.numpy().ctypes.data_as(C.c_void_p), ids.numel(), C.c_uint64(key),
                                          C.byref(out)), "dtk_slot_lcp")
        return int(out.value)

    def best_lcp_slot(self, slots: Iterable[int], ids: torch.Tensor, key: int = 0) -> Optional[Tuple[int, int]]:
        """(slot, lcp) of the slot among `slots` whose cache shares the longest prefix with ids (lowest index on ties), None if
        none shares a token"""
        ids = ids.detach().to("cpu", torch.int64).reshape(-1).contiguous()
        ptr, n, out, best = ids.numpy().ctypes.data_as(C.c_void_p), ids.numel(), C.c_int(0), None
        for s_ in slots:
            self._check(self.lib.dtk_slot_lcp(self._ctx, int(s_), ptr, n, C.c_uint64(key), C.byref(out)), "dtk_slot_lcp")
            if out.value > (best[1] if best else 0):
                best = (int(s_), int(out.value))
        return best

    def cached_ids(self, slot: int, n_max: int = 4096) -> List[int]:
        out = (C.c_int64 * n_max)()
        n = self.lib.dtk_slot_cached_ids(self._ctx, int(slot), out, n_max)
        return [int(out[i]) for i in range(max(0, n))]

    def resume_slot(self, slot: int, ids: torch.Tensor, key: int = 0):
        ids = ids.detach().to("cpu", torch.int64).reshape(-1).contiguous()
        self._check(self.lib.dtk_resume_slot(self._ctx, int(slot), ids.numpy().ctypes.data_as(C.c_void_p), ids.numel(), C.c_uint64(key)),
                    "dtk_resume_slot")

    def get_logits_slot(self, slot: int) -> torch.Tensor:
        out = np.empty(self.config.vocab, dtype=np.float32)
        self._check(self.lib.dtk_get_logits_slot(self._ctx, int(slot), out.ctypes.data_as(C.c_void_p)), "dtk_get_logits_slot")
        return torch.from_numpy(out)

    def context_len_slot(self, slot: int) -> int:
        return int(self.lib.dtk_context_len_slot(self._ctx, int(slot)))

    @property
    def kv_format(self) -> str:
        """ "bf16" or "mxfp8": the format in which the batched decode steps read the rows that decode steps wrote (load(kv_format=))"""
        return getattr(self.config, "kv_format", "bf16")

    def kv8_from(self, slot: int) -> int:
        """kv_format "mxfp8": the first row of the slot that its decode steps read as MXFP8 (the rows below it are prefill or forked
        rows and exist in bf16 only).  A bf16 context raises DtkError."""
        out = C.c_int(0)
        self._check(self.lib.dtk_kv8_info(self._ctx, int(slot), C.byref(out)), "dtk_kv8_info")
        return int(out.value)

    def read_kv8(self, slot: int, layer: int, which: int, row0: int, nrows: int):
        """diagnostic (kv_format "mxfp8"): (codes uint8 [KVH, nrows, 128], scales uint8 [KVH, nrows, 4], bf16 rows [KVH, nrows, 128]) of
        rows [row0, row0 + nrows) of a layer's keys (which = 0) or values (1) in a decoding slot"""
        kvh = int(getattr(self.config, "kv_heads", 0) or 0) or int(self.config.heads)
        codes = torch.empty(kvh, nrows, 128, dtype=torch.uint8)
        scales = torch.empty(kvh, nrows, 4, dtype=torch.uint8)
        rows = torch.empty(kvh, nrows, 128, dtype=torch.int16)
        self._check(self.lib.dtk_read_kv8(self._ctx, int(slot), int(layer), int(which), int(row0), int(nrows),
                                          C.c_void_p(codes.data_ptr()), C.c_void_p(scales.data_ptr()), C.c_void_p(rows.data_ptr())), "dtk_read_kv8")
        return codes, scales, rows.view(torch.bfloat16)

    def decode_launch(self):
        self._check(self.lib.dtk_decode_launch(self._ctx), "dtk_decode_launch")

    def decode_wait(self, top: bool = False):
        """the token of the oldest unread step.  top=True (needs enable_top_logprobs(k)): (token, logprob, sample_logprob, top_ids,
        top_logprobs), the last two lists of k entries ((-1, NaN) for a forced token)"""
        tok = C.c_int64()
        if top:
            lp, k = (C.c_float * 2)(), self.top_logprobs_enabled
            ti, tl = (C.c_int32 * _lib.DTK_MAX_TOP)(), (C.c_float * _lib.DTK_MAX_TOP)()
            self._check(self.lib.dtk_decode_wait_top(self._ctx, C.byref(tok), lp, ti, tl), "dtk_decode_wait_top")
            return int(tok.value), float(lp[0]), float(lp[1]), list(ti[:k]), list(tl[:k])
        self._check(self.lib.dtk_decode_wait(self._ctx, C.byref(tok)), "dtk_decode_wait")
        return int(tok.value)

    def decode_wait_lp(self) -> Tuple[int, float, float]:
        """decode_wait + the token's (logprob, sample_logprob); needs enable_logprobs()"""
        tok, lp = C.c_int64(), (C.c_float * 2)()
        self._check(self.lib.dtk_decode_wait_lp(self._ctx, C.byref(tok), lp), "dtk_decode_wait_lp")
        return int(tok.value), float(lp[0]), float(lp[1])

    def get_logits(self) -> torch.Tensor:
        out = np.empty(self.config.vocab, dtype=np.float32)
        self._check(self.lib.dtk_get_logits(self._ctx, out.ctypes.data_as(C.c_void_p)), "dtk_get_logits")
        return torch.from_numpy(out)

    def context_len(self) -> int:
        return int(self.lib.dtk_context_len(self._ctx))

    def set_graph_mode(self, mode: int):
        self._check(self.lib.dtk_set_graph_mode(self._ctx, int(mode)), "dtk_set_graph_mode")

    def set_option(self, name: str, value: int):
        self._check(self.lib.dtk_set_option(self._ctx, name.encode(), int(value)), f"dtk_set_option({name})")

    def synchronize(self):
        self._check(self.lib.dtk_synchronize(self._ctx), "dtk_synchronize")

    def stats(self) -> Dict[str, Any]:
        st = _lib.DtkStats()
        self._check(self.lib.dtk_get_stats(self._ctx, C.byref(st)), "dtk_get_stats")
        return {k: getattr(st, k) for k, _ in st._fields_}

    # ---- generation ---------------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, input_ids: Optional[torch.Tensor] = None, pixel_values: Optional[torch.Tensor] = None,
                 bad_words_ids: Optional[List[List[int]]] = None,
                 begin_suppress_tokens: Optional[List[int]] = None,
                 suppress_tokens: Optional[List[int]] = None,
                 streamer=None, stopping_criteria=None, do_sample: Optional[bool] = None,
                 temperature: Optional[float] = None, top_p: Optional[float] = None,
                 top_k: Optional[int] = None, max_length: Optional[int] = None,
                 max_new_tokens: Optional[int] = None, eos_token_id=None, seed: Optional[int] = None,
                 inputs: Optional[torch.Tensor] = None, sequence_owner: Optional[int] = None, return_logprobs: bool = False,
                 top_logprobs: Optional[int] = None, min_p: Optional[float] = None, epsilon_cutoff: Optional[float] = None,
                 presence_penalty: Optional[float] = None, frequency_penalty: Optional[float] = None,
                 penalty_start: Optional[int] = None, dry_multiplier: Optional[float] = None, dry_base: Optional[float] = None,
                 dry_allowed_length: Optional[int] = None, dry_start: Optional[int] = None, dry_sequence_breakers=None,
                 min_new_tokens: Optional[int] = None, exponential_decay_length_penalty=None, logit_bias=None, sequence_bias=None,
                 length_start: Optional[int] = None, guidance_scale: Optional[float] = None,
                 negative_prompt_ids: Optional[torch.Tensor] = None, negative_pixel_values: Optional[torch.Tensor] = None,
                 negative_adapter_input_ids: Optional[torch.Tensor] = None, prompt_lookup_num_tokens: Optional[int] = None,
                 max_matching_ngram_size: Optional[int] = None, prompt_lookup_drafts: Optional[Sequence[int]] = None,
                 prompt_lookup_corpus=None, **hf_kwargs) -> Union[torch.Tensor, GenerateOutput]:
        """One sequence of HF GenerationMixin.generate/_sample semantics (generation/utils.py
        :2783-2950): streamer.put(prompt) once, then per token: processors -> argmax|draw ->
        append -> streamer.put(token) -> stopping criteria (max length, EOS, user criteria);
        streamer.end().  Returns (1, T') int64 on the host.

        return_logprobs=True (not an HF argument; HF's output_scores / compute_transition_scores stay refused) returns a
        GenerateOutput instead: the same tensor as `.sequences` plus the per-token `.logprobs` / `.sample_logprobs` the sampler
        kernel formed on its way (enable_logprobs(): switched on for this call if needed, and left on).  top_logprobs=k (1 .. 8,
        with return_logprobs=True): + `.top_ids` / `.top_logprobs`, the k most likely tokens at every new position; under a batch engine only
        one built with top_logprobs >= k (NativeBatchEngine / make_engine(..., top_logprobs=)).  Without an engine the option is on for this call only.

        min_p / epsilon_cutoff: HF's MinPLogitsWarper / EpsilonLogitsWarper behind top-p (HF's order), as thresholds on the sampler's
        integer masses; 0 / None = off; ignored by greedy decoding like temperature, top-k and top-p.

        presence_penalty / frequency_penalty: the OpenAI / vLLM pair, in [-2, 2], 0 / None = off: every id that occurs c > 0 times
        among the sequence's tokens from position penalty_start on (default: the prompt length, so only generated tokens count) has
        presence + frequency * c taken off its raw logit in front of the whole sampler chain, greedy included.  The
        reported log-probabilities stay the model's own.  HF's repetition_penalty stays refused.

        dry_multiplier / dry_base / dry_allowed_length / dry_start / dry_sequence_breakers: DRY (text-generation-webui, llama.cpp): the
        token that would extend a verbatim repetition of M >= dry_allowed_length (default 2) tokens of the sequence's own text from
        position dry_start on (default: the prompt length) has dry_multiplier * dry_base^(M - dry_allowed_length) taken off its logit,
        behind the presence / frequency pair and in front of everything else; dry_multiplier 0 / None = off; breakers
        are token ids across which no repetition is matched.  The reported log-probabilities stay the model's own.

        min_new_tokens / exponential_decay_length_penalty=(start, factor): HF's MinNewTokensLength processor (the EOS logits are -inf
        until the sequence holds min_new_tokens tokens behind position length_start) and its ExponentialDecayLengthPenalty (from
        start + 1 tokens on the EOS logits grow by |z| * (factor^k - 1)); length_start defaults to the prompt length.  logit_bias={id:
        value} (OpenAI / vLLM) and HF's sequence_bias with single-token sequences: one table of at most 256 biases in [-100, 100] added
        to the raw logits in front of the penalties.  0 / None = off.  The reported log-probabilities stay the model's own.

        guidance_scale=g (HF's UnbatchedClassifierFreeGuidanceLogitsProcessor; a finite number in [0, 100]; None / 1 = off): classifier-free
        guidance against a negative prompt — negative_prompt_ids (default: input_ids, so a rollout that continues a node carries the program
        text so far in both branches), negative_pixel_values (default: pixel_values) and, with an adapter, negative_adapter_input_ids
        (default: no text).  At least one of the three must be given: the negative branch has to differ in something.  The two sequences
        decode as a pair in slots 0 and 1 of a model loaded with batch_slots >= 2, one pass over the weights for both; every step the raw
        logits become g * (log_softmax(z) - log_softmax(z_neg)) + log_softmax(z_neg) on the device, in front of EVERYTHING else: the
        alternatives of top_logprobs, logit_bias, the penalties, DRY, the length rules, the suppression lists, temperature, top-k,
        top-p, min-p, epsilon, greedy included (HF's processor order).  Consequently `.logprobs`, `.top_ids` and
        `.top_logprobs` of a guided call describe the GUIDED distribution (out[t] - logsumexp(out)), not the model's own.  Not in the
        batch engines yet, unless the engine was built with guided_pairs=P (the pair then decodes in two of the engine's slots, the same
        tokens and log-probabilities); contexts without slots (tl-1.1b, MXFP4) have no guidance.

        prompt_lookup_num_tokens=K (HF's name; 1 .. 3, None / 0 = off) with max_matching_ngram_size (default 2): prompt-lookup
        speculative decoding.  The sequence decodes in SLOT 0 of a model loaded with batch_slots = K + 1 .. 5: one
        multi-vector step verifies up to K drafted tokens — the continuation of the earlier occurrence of the sequence's last n-gram,
        HF's PromptLookupCandidateGenerator — and accepts 1 .. K + 1 tokens.  Tokens, `.logprobs` and `.sample_logprobs` are, bit for
        bit, what plain steps of slot 0 on the same context (decode_batch_launch([0])) give, greedy or sampled; a call WITHOUT the
        argument runs the single-sequence step, whose kernels differ, so no identity with it (or with a batch_slots=0 context) is
        claimed — classifier-free guidance lives with the same fact.  `.accepted_per_step` of the GenerateOutput lists what every step
        accepted.  Not with guidance, penalties, DRY, the length rules, a bias, top_logprobs, kv_format mxfp8 or a batch engine
        (NotImplementedError).  prompt_lookup_drafts (not an HF argument; tests): an id per absolute position, -1 = none, used as the
        drafts instead of the lookup.  prompt_lookup_corpus=[seq, ...] (not an HF argument; retrieval-based drafting as in REST): 1-D id
        sequences, lists or tensors — earlier programs of the same image, tokenised boilerplate — as a second place to look.  At every
        n-gram size the sequence's own ids are searched first, then the corpus (first window whose continuation holds an id; a window
        never spans two sequences); a longer n-gram beats a shorter one whatever its source.  The verify pass decides every token, so
        the output is the same with any corpus; `.draft_sources` = (history, corpus, none) counts the steps by where their drafts came
        from.  The corpus is set for this call alone.  ValueError without prompt_lookup_num_tokens, for ids outside the vocabulary,
        and when the ids plus one separator between sequences exceed 65536 entries; empty sequences are dropped.

        Any other HF generation argument is accepted only at the value that leaves `_sample` unchanged
        (`_NEUTRAL_GENERATE_KWARGS`); everything else — beams, penalties, several return sequences, constraints,
        unknown names — raises instead of being dropped: a drop-in must not silently decode something else."""
        topk = check_top_logprobs(top_logprobs, return_logprobs)
        if guidance_scale is not None:      # (a bad value raises before anything else is looked at)
            check_guidance_scale(guidance_scale)
        if prompt_lookup_num_tokens is not None or max_matching_ngram_size is not None:      # (likewise)
            check_prompt_lookup(prompt_lookup_num_tokens, max_matching_ngram_size)
        if not self._weights_ready:
            raise _lib.DtkError("no weights loaded (load_state_dict / fill_synthetic first)")
        text_ids = None
        if "adapter_input_ids" in hf_kwargs or "adapter_attention_mask" in hf_kwargs:
            if not self.has_adapter():
                raise TypeError("generate() got adapter_input_ids / adapter_attention_mask but no adapter is loaded "
                                "(load(..., adapter=True))")
            tids, tmask = hf_kwargs.pop("adapter_input_ids", None), hf_kwargs.pop("adapter_attention_mask", None)
            if tids is None and tmask is not None:
                raise ValueError("adapter_attention_mask without adapter_input_ids")
            if tids is not None:
                text_ids = adapter_text(tids, tmask)
        _reject_unsupported_generate_kwargs(hf_kwargs)
        guide = check_guidance_scale(getattr(self.generation_config, "guidance_scale", None) if guidance_scale is None else guidance_scale)
        guided = guide != 1.0
        if guided:      # everything that refuses a guided call, before anything runs
            if negative_prompt_ids is None and negative_pixel_values is None and negative_adapter_input_ids is None:
                raise ValueError(f"guidance_scale = {guide}: the negative branch must differ from the prompt in something — pass "
                                 "negative_prompt_ids, negative_pixel_values and / or negative_adapter_input_ids")
            if self.batch_engine is not None and not getattr(self.batch_engine, "guided_pairs", 0):
                raise NotImplementedError("guidance_scale: not in the batch engines yet — unless the engine was built for it "
                                          "(NativeBatchEngine / make_engine(..., guided_pairs=P))")
            if self.num_slots() < 2:
                raise ValueError("guidance_scale needs two batch slots for the guided pair: load(..., batch_slots=2) or more "
                                 "(contexts without slots — tl-1.1b, MXFP4 — have no guidance)")
            if self.batch_engine is None:
                self._refuse_while_batch_busy("generate")
        spec_k, spec_n = check_prompt_lookup(
            getattr(self.generation_config, "prompt_lookup_num_tokens", None) if prompt_lookup_num_tokens is None else prompt_lookup_num_tokens,
            getattr(self.generation_config, "max_matching_ngram_size", None) if max_matching_ngram_size is None else max_matching_ngram_size)
        if prompt_lookup_drafts is not None and not spec_k:
            raise ValueError("prompt_lookup_drafts without prompt_lookup_num_tokens")
        if prompt_lookup_corpus is not None and not spec_k:
            raise ValueError("prompt_lookup_corpus without prompt_lookup_num_tokens")
        corpus = flatten_corpus(prompt_lookup_corpus, int(self.config.vocab))
        if spec_k:      # everything that refuses a speculative call, before anything runs
            if guided:
                raise NotImplementedError("prompt_lookup_num_tokens: not together with guidance_scale (the guided pair needs the step's slots)")
            if topk:
                raise NotImplementedError("prompt_lookup_num_tokens: not together with top_logprobs (its records are per slot and step)")
            if self.batch_engine is not None:
                raise NotImplementedError("prompt_lookup_num_tokens: not in the batch engines (the speculative step takes the "
                                          "multi-vector step's slots for one sequence)")
            if self.num_slots() < spec_k + 1:
                raise ValueError(f"prompt_lookup_num_tokens = {spec_k} needs {spec_k + 1} batch slots for the positions one step verifies: "
                                 f"load(..., batch_slots={spec_k + 1}) up to 5 (contexts without slots — tl-1.1b, MXFP4 — do not speculate)")
            if self.num_slots() > 5:
                raise NotImplementedError(f"prompt_lookup_num_tokens: not on a context with {self.num_slots()} batch slots (the verify pass is the "
                                          "multi-vector step of contexts with 2 .. 5 slots: load(..., batch_slots=4))")
            if self.kv_format != "bf16":
                raise NotImplementedError("prompt_lookup_num_tokens: not with kv_format mxfp8 (the positions of a step share slot 0's rows)")
            self._refuse_while_batch_busy("generate")
        if input_ids is None:
            input_ids = inputs
        ids = input_ids.detach().to("cpu", torch.int64)
        if ids.dim() == 1:
            ids = ids[None]
        if ids.shape[0] != 1:
            raise ValueError("batch size 1 only (the reference generates one sequence per call)")
        neg_ids = neg_px = neg_text = None
        if guided:
            neg_ids = ids if negative_prompt_ids is None else negative_prompt_ids.detach().to("cpu", torch.int64).reshape(1, -1)
            neg_px = pixel_values if negative_pixel_values is None else negative_pixel_values
            if negative_adapter_input_ids is not None:
                if not self.has_adapter():
                    raise TypeError("generate() got negative_adapter_input_ids but no adapter is loaded (load(..., adapter=True))")
                neg_text = adapter_text(negative_adapter_input_ids)
            if neg_px is None and neg_text is None:
                raise ValueError("guidance_scale with a text-only prompt: the adapter's dummy input cannot be prefilled without a text, so "
                                 "the negative branch needs one of its own — pass negative_adapter_input_ids (the pipeline's negative_text)")
        gc = self.generation_config
        min_p, epsilon_cutoff = check_truncation(getattr(gc, "min_p", None) if min_p is None else min_p,
                                                 getattr(gc, "epsilon_cutoff", None) if epsilon_cutoff is None else epsilon_cutoff)
        presence_penalty, frequency_penalty, penalty_start = check_penalties(
            getattr(gc, "presence_penalty", None) if presence_penalty is None else presence_penalty,
            getattr(gc, "frequency_penalty", None) if frequency_penalty is None else frequency_penalty,
            getattr(gc, "penalty_start", None) if penalty_start is None else penalty_start)
        dry_multiplier, dry_base, dry_allowed_length, dry_start, dry_sequence_breakers = check_dry(
            getattr(gc, "dry_multiplier", None) if dry_multiplier is None else dry_multiplier,
            getattr(gc, "dry_base", None) if dry_base is None else dry_base,
            getattr(gc, "dry_allowed_length", None) if dry_allowed_length is None else dry_allowed_length,
            getattr(gc, "dry_start", None) if dry_start is None else dry_start,
            getattr(gc, "dry_sequence_breakers", None) if dry_sequence_breakers is None else dry_sequence_breakers,
            int(self.config.vocab))
        min_new_tokens, decay, length_start = check_length_control(
            getattr(gc, "min_new_tokens", None) if min_new_tokens is None else min_new_tokens,
            getattr(gc, "exponential_decay_length_penalty", None) if exponential_decay_length_penalty is None else exponential_decay_length_penalty,
            getattr(gc, "length_start", None) if length_start is None else length_start)
        bias_pairs = check_logit_bias(getattr(gc, "logit_bias", None) if logit_bias is None else logit_bias,
                                      getattr(gc, "sequence_bias", None) if sequence_bias is None else sequence_bias, int(self.config.vocab))
        if spec_k:      # their tables depend on the position: they come later
            for name, on in (("presence_penalty / frequency_penalty", presence_penalty or frequency_penalty), ("dry_multiplier", dry_multiplier),
                             ("min_new_tokens / exponential_decay_length_penalty", min_new_tokens or decay),
                             ("logit_bias / sequence_bias", bias_pairs)):
                if on:
                    raise NotImplementedError(f"prompt_lookup_num_tokens: not together with {name} yet")
        do_sample = gc.do_sample if do_sample is None else do_sample
        temperature = gc.temperature if temperature is None else temperature
        top_p = gc.top_p if top_p is None else top_p
        top_k = gc.top_k if top_k is None else top_k
        T = ids.shape[1]
        if length_start is None:
            length_start = T
        if penalty_start is None:
            penalty_start = T
        if dry_start is None:
            dry_start = T
        dry = dict(dry_multiplier=dry_multiplier, dry_base=dry_base, dry_allowed_length=dry_allowed_length, dry_start=dry_start,
                   dry_sequence_breakers=dry_sequence_breakers) if dry_multiplier else {}
        if max_new_tokens is not None:
            max_length = T + int(max_new_tokens)
        elif max_length is None:
            max_length = gc.max_length
        max_length = min(int(max_length), self.config.max_positions)
        if guided and neg_ids.shape[1] > T:      # both sequences grow by the same tokens: the longer prompt bounds the new ones
            max_length = min(max_length, T + self.config.max_positions - int(neg_ids.shape[1]))
        eos = eos_token_id if eos_token_id is not None else gc.eos_token_id
        eos_set = set(_flat_ids([eos]))
        # the length rules act on the valid EOS ids (none, as with eos_token_id=-1: nothing to do)
        len_eos = length_eos_ids(eos_set, int(self.config.vocab)) if (min_new_tokens or decay) else ()
        shape = {}
        if len_eos:
            shape.update(min_new_tokens=min_new_tokens, exponential_decay_length_penalty=decay, length_start=length_start, length_eos_ids=len_eos)
        if bias_pairs:
            shape.update(logit_bias=bias_pairs)
        begin_suppress_tokens = _flat_ids(begin_suppress_tokens)
        suppress_tokens = _flat_ids(suppress_tokens)
        bad = []
        for w in (bad_words_ids or []):
            if len(w) != 1:
                raise NotImplementedError("multi-token bad words are not used by DeTikZify")
            bad.append(int(w[0]))
        if seed is None:  # reproducible under torch.manual_seed / transformers.set_seed, like HF
            seed = int(torch.randint(0, 2 ** 62, (), dtype=torch.int64).item()) if do_sample else 0

        if streamer is not None:
            streamer.put(ids.cpu())
        criteria = list(stopping_criteria) if stopping_criteria is not None else []
        n_new_max = max_length - T
        buf = torch.empty((1, max(max_length, T)), dtype=torch.int64)
        buf[0, :T] = ids[0]
        cur = T
        # per-token host work (runs under the GPU's next step): append, stream, stopping criteria.  Kept light: 32 rollouts
        # share one GIL.  The token tensor the HF protocols expect is only built for callers that need it.
        put_token = getattr(streamer, "put_token", None) if streamer is not None else None
        from ..util.generation import ExplicitAbort
        light = [c for c in criteria if type(c) is ExplicitAbort]        # polled flag: ignores its arguments
        heavy = [c for c in criteria if type(c) is not ExplicitAbort]
        new_tokens: List[int] = []
        pairs: Tuple[List[float], List[float]] = ([], [])      # return_logprobs: one pair per delivered token (trimmed to new_tokens)
        tops: Tuple[List[List[int]], List[List[float]]] = ([], [])      # top_logprobs: k ids and k log-probabilities per delivered token

        def emit(tok: int) -> bool:
            nonlocal cur
            new_tokens.append(tok)
            cur += 1
            if put_token is not None:
                put_token(tok)
            elif streamer is not None:
                streamer.put(torch.tensor([tok], dtype=torch.int64))
            stop = tok in eos_set or cur >= max_length
            for c in light:
                stop = stop or c.should_stop
            if heavy:
                buf[0, cur - 1] = tok
                for crit in heavy:
                    r = crit(buf[:, :cur], None)
                    stop = stop or bool(r.all() if isinstance(r, torch.Tensor) else r)
            return stop

        put_tokens = getattr(streamer, "put_tokens", None) if streamer is not None else None

        def emit_many(toks: List[int]) -> bool:
            """the tokens of consecutive steps (a multi-step engine run): the same effects, in order, as emit() per token.  The
            polled abort flag is looked at once per call — a consumer that quits stops the sequence at most one run later."""
            nonlocal cur
            if heavy or (streamer is not None and put_token is None):
                for tok in toks:            # arbitrary criteria / foreign streamers keep the per-token protocol
                    if emit(tok):
                        return True
                return False
            n, stop = 0, False
            for tok in toks:
                n += 1
                if tok in eos_set or cur + n >= max_length:
                    stop = True
                    break
            chunk = toks[:n]
            new_tokens.extend(chunk)
            cur += n
            if put_tokens is not None:
                put_tokens(chunk)
            elif put_token is not None:
                for tok in chunk:
                    put_token(tok)
            for c in light:
                stop = stop or c.should_stop
            return stop

        emit.many, emit.budget, emit.stop_ids = emit_many, (lambda: max_length - cur), eos_set
        emit.aborted = lambda: any(c.should_stop for c in light)
        engine = self.batch_engine
        if n_new_max > 0 and engine is not None:
            # batched mode: this sequence decodes in a KV slot together with the other threads' sequences (infer/engine.py: the
            # native run loop; infer/batching.py: the Python-driven one); one pass over the weights serves all of them.  The
            # sequence's own end (EOS, length budget) goes with it: the native loop stops the slot there.  Tokens come back in
            # bursts (one per source line) unless something here needs to see every token as it is made.  A text (the adapter)
            # goes with the sequence: its slot's prefix is keyed by (image, text).
            per_token = bool(heavy) or (streamer is not None and (put_token is None or bool(getattr(streamer, "per_token", put_tokens is None))))
            with engine.sequence(ids[0], pixel_values, dict(
                    do_sample=do_sample, temperature=temperature, top_p=top_p, top_k=top_k, seed=seed, bad_ids=bad,
                    begin_suppress_ids=begin_suppress_tokens or (), always_suppress_ids=suppress_tokens or (),
                    **({"min_p": min_p, "epsilon_cutoff": epsilon_cutoff} if (min_p or epsilon_cutoff) else {}),
                    **({"presence_penalty": presence_penalty, "frequency_penalty": frequency_penalty, "penalty_start": penalty_start}
                       if (presence_penalty or frequency_penalty) else {}), **dry, **shape),
                    owner=sequence_owner, max_new_tokens=n_new_max, stop_ids=eos_set, per_token=per_token, text_ids=text_ids,
                    **({"logprobs": True} if return_logprobs else {}), **({"top_logprobs": topk} if topk else {}),
                    **({"guidance": dict(scale=guide, ids=neg_ids[0], pixel_values=neg_px, text_ids=neg_text)} if guided else {})) as seq:
                seq.run(emit)       # emit.many() per burst in this thread (native engine) / emit() per token by the driving thread
                if return_logprobs:
                    pairs = (seq.logprobs, seq.sample_logprobs)
                if topk:
                    tops = (seq.top_ids, seq.top_logprobs)
        elif n_new_max > 0:
            # the context has ONE un-slotted sequence: a second generate() on it from another thread would interleave its
            # prefill / decode steps with ours and both would return garbage — refuse loudly (the reference never does
            # this either; concurrent rollouts go through a BatchEngine)
            if not self._single_busy.acquire(blocking=False):
                raise _lib.DtkError("concurrent generate() calls on one model: decode them as a batch "
                                    "(detikzify_amd.infer.batching.BatchEngine / simulate_parallel)")
            launched = received = 0
            at = {"slot": 0} if (guided or spec_k) else {}      # a guided pair decodes in slots 0 (this call's sampling state) and 1 (the negative prompt); a speculating sequence in slot 0
            spec_open, accepted = False, []
            corpus_set, sources = False, None
            try:
                self.set_sampling(do_sample, temperature, top_p, top_k, seed, bad,
                                  begin_suppress_tokens or (), suppress_tokens or (), **at)
                if min_p or epsilon_cutoff:       # (set_sampling reset both)
                    self.set_sampling_ext(min_p, epsilon_cutoff, **at)
                if presence_penalty or frequency_penalty:       # (likewise; the prefill below builds the count table)
                    self.set_penalties(presence_penalty, frequency_penalty, penalty_start, **at)
                if dry_multiplier:       # (likewise; the prefill below builds the history)
                    self.set_dry(dry_multiplier, dry_base, dry_allowed_length, dry_start, dry_sequence_breakers, **at)
                if len_eos:              # (likewise; static for the sequence: the length comes from the device's own position)
                    self.set_length_control(min_new_tokens, decay, length_start, len_eos, **at)
                if bias_pairs:
                    self.set_logit_bias(bias_pairs, **at)
                if guided:               # the unconditional slot: neutral greedy sampling, no tables (its own choice is never used)
                    self.set_sampling(slot=1)
                if return_logprobs:       # (after set_sampling: steps an earlier call left unread are forgotten there, the switch refuses them)
                    self.enable_logprobs()
                    if topk:
                        self.enable_top_logprobs(topk)
                if text_ids is not None:
                    self.prefill(ids[0], pixel_values, adapter_input_ids=text_ids, **at)
                else:
                    self.prefill(ids[0], pixel_values, **at)
                if guided:
                    if neg_text is not None:
                        self.prefill(neg_ids[0], neg_px, adapter_input_ids=neg_text, slot=1)
                    else:
                        self.prefill(neg_ids[0], neg_px, slot=1)
                    self.set_guidance(guide, 0, 1)

                launched = received = 0
                stop = False
                ahead = 2  # one step always in flight while the host handles the previous token
                if spec_k:      # the same pipelining over speculative steps: every step read hands over 1 .. K + 1 tokens
                    if corpus:      # the second draft source, for this call alone (cleared where the speculation ends)
                        self._spec_set_corpus(corpus)
                        corpus_set = True
                    self.spec_begin(spec_k, spec_n, table=prompt_lookup_drafts is not None)
                    spec_open = True
                    if prompt_lookup_drafts is not None:
                        self.spec_set_drafts(prompt_lookup_drafts)
                    inflight = 0
                    while not stop:
                        # a step in flight yields at least one token and moves the position by at most four (the library's own bound)
                        while (inflight < ahead and len(new_tokens) + inflight < n_new_max
                               and cur + 4 * inflight < self.config.max_positions):
                            self.spec_launch(); inflight += 1
                        if not inflight:
                            break
                        got = self.spec_wait(logprobs=return_logprobs); inflight -= 1
                        toks = got[0] if return_logprobs else got
                        accepted.append(len(toks))
                        for i, tok in enumerate(toks):      # the streamer sees them one by one; what lies behind the stop is dropped
                            if return_logprobs:
                                pairs[0].append(got[1][i]); pairs[1].append(got[2][i])
                            stop = emit(tok)
                            if stop:
                                break
                    launched = received = n_new_max      # (the plain loops below have nothing to do)
                if guided:      # the same loop over steps of the pair: slot 0's token and records are the sequence's
                    while launched < min(ahead, n_new_max):
                        self.decode_batch_launch([0, 1]); launched += 1
                    while received < launched:
                        if topk:
                            toks, lps, slps, tis, tls = self.decode_batch_wait(top=True)
                            pairs[0].append(lps[0]); pairs[1].append(slps[0]); tops[0].append(tis[0]); tops[1].append(tls[0])
                        elif return_logprobs:
                            toks, lps, slps = self.decode_batch_wait_lp()
                            pairs[0].append(lps[0]); pairs[1].append(slps[0])
                        else:
                            toks = self.decode_batch_wait()
                        received += 1
                        if toks[0] != toks[1]:      # the follower hands slot 1 the token slot 0's chain chose: one token per pair per step
                            raise _lib.DtkError(f"guided pair: slot 0 reports token {toks[0]}, slot 1 token {toks[1]}")
                        stop = emit(toks[0])
                        if stop:
                            break
                        if launched < n_new_max:
                            self.decode_batch_launch([0, 1]); launched += 1
                while not guided and launched < min(ahead, n_new_max):
                    self.decode_launch(); launched += 1
                while not guided and received < launched:
                    if topk:
                        tok, lp, slp, ti, tl = self.decode_wait(top=True)
                        pairs[0].append(lp); pairs[1].append(slp); tops[0].append(ti); tops[1].append(tl)
                    elif return_logprobs:
                        tok, lp, slp = self.decode_wait_lp()
                        pairs[0].append(lp); pairs[1].append(slp)
                    else:
                        tok = self.decode_wait()
                    received += 1
                    stop = emit(tok)
                    if stop:
                        break
                    if launched < n_new_max:
                        self.decode_launch(); launched += 1
            finally:
                try:
                    try:
                        if spec_open:      # the steps in flight are read, slot 0 keeps exactly the sequence as returned (no pending logits)
                            self.spec_end(cur)
                            if corpus_set:
                                sources = self.spec_counters()
                    finally:
                        if corpus_set:     # a later call without the argument sees no corpus
                            self._spec_set_corpus([])
                    if topk or guided:      # the call that asked for the alternatives / the pair switches them off again: later steps run without the extra kernels
                        self.synchronize()
                        while received < launched:      # (a step left in flight behind the last token: the switches refuse unread steps)
                            received += 1
                            if guided:
                                self.decode_batch_wait()
                            else:
                                self.decode_wait()
                        if guided:
                            self.set_guidance(None, 0, None)
                        if topk:
                            self.enable_top_logprobs(0)
                finally:
                    self._single_busy.release()
        if streamer is not None:
            streamer.end()
        if new_tokens:
            buf[0, T:T + len(new_tokens)] = torch.tensor(new_tokens, dtype=torch.int64)
        if return_logprobs:       # (an engine may have delivered pairs of tokens past the sequence's end: the first len(new_tokens) are its own)
            n = len(new_tokens)
            out = GenerateOutput(buf[:, :cur].clone(), torch.tensor(pairs[0][:n], dtype=torch.float32)[None],
                                  torch.tensor(pairs[1][:n], dtype=torch.float32)[None],
                                  torch.tensor(tops[0][:n], dtype=torch.int64).reshape(1, n, topk) if topk else None,
                                  torch.tensor(tops[1][:n], dtype=torch.float32).reshape(1, n, topk) if topk else None)
            if spec_k and engine is None and n_new_max > 0:
                out.accepted_per_step = accepted
                out.draft_sources = sources
            return out
        return buf[:, :cur].clone()
