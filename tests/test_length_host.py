"""Length control and logit bias without a GPU: the specification (tests/shape_oracle.py) against the installed transformers' three logits
processors bit for bit, the saturation of the decay table, generate()'s argument gate, the additive C ABI, and the calls of both batch
engines and of DetikzifyGenerator over the scripted device."""
from __future__ import annotations

import ctypes as C
import math
import re
import struct
from pathlib import Path

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from detikzify_amd.infer.batching import BatchEngine
from detikzify_amd.infer.engine import NativeBatchEngine
from detikzify_amd.model.modeling import check_length_control, check_logit_bias

from . import shape_oracle
from .helpers import fake_processor
from .test_generate_loop import EOS, IMG, NIMG, VOCAB, ScriptedDevice, _prompt

HEADER = (Path(__file__).resolve().parents[1] / "include" / "dtk.h").read_text()


def _bits(x) -> int:
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


# ------------------------------------------------------------------------------------------ the rule
V = 1000
FACTORS = (0.9, 1.01, 1.3, 2.0)
STARTS = (0, 3)


def _rows():
    g = torch.Generator().manual_seed(20261)
    rows = (torch.randn(6, V, generator=g) * 6.0).to(torch.float32)
    rows[1, 7] = -3.25          # a negative EOS logit
    rows[2, 7] = 0.0            # ... and one of exactly 0
    rows[3, 7] = -0.0
    return rows


def test_oracle_equals_hf_processors_bit_for_bit():
    from transformers.generation.logits_process import (ExponentialDecayLengthPenalty, MinNewTokensLengthLogitsProcessor,
                                                        SequenceBiasLogitsProcessor)
    rows = _rows()
    eos = [7, V - 1]
    prompt = 11
    compared = 0
    for factor in FACTORS:
        for dstart in STARTS:
            for min_new in (0, dstart):             # (decay_start >= min_new_tokens)
                decay = ExponentialDecayLengthPenalty((dstart, factor), eos, prompt)
                minlen = MinNewTokensLengthLogitsProcessor(prompt, min_new, eos)
                # n across both thresholds: min_new - 1, min_new, decay_start, decay_start + 1, and on into the decay
                for n in sorted({max(min_new - 1, 0), min_new, dstart, dstart + 1, dstart + 2, dstart + 9, dstart + 40}):
                    cur = prompt + n
                    ids = torch.zeros((1, cur), dtype=torch.int64)
                    for row in rows:
                        want = minlen(ids, decay(ids, row[None].clone()))[0]
                        got = shape_oracle.eos_rules(row, cur, eos, min_new, (dstart, factor), start=prompt)
                        assert _same_bits(got, want), (factor, dstart, min_new, n)
                        compared += 1
                        other = [i for i in range(V) if i not in eos]
                        assert _same_bits(got[other], row[other])          # nothing but E moves
    assert compared >= 300
    # rule 1 against SequenceBiasLogitsProcessor (single-token sequences)
    pairs = {3: 2.5, 7: -100.0, V - 1: 100.0, 500: 1e-3, 501: -7.0}
    proc = SequenceBiasLogitsProcessor({(t,): float(v) for t, v in pairs.items()})
    ids = torch.zeros((1, 5), dtype=torch.int64)
    for row in rows:
        assert _same_bits(shape_oracle.bias(row, pairs), proc(ids, row[None].clone())[0])
    # a bias of 0 leaves the bits alone (-0.0 stays -0.0)
    assert _bits(shape_oracle.bias(rows[3], {7: 0.0})[7]) == 0x80000000
    # the whole chain in HF's order of these three: bias, decay, minimum
    decay, minlen = ExponentialDecayLengthPenalty((3, 1.3), eos, prompt), MinNewTokensLengthLogitsProcessor(prompt, 2, eos)
    for n in (0, 1, 2, 3, 4, 12):
        ids = torch.zeros((1, prompt + n), dtype=torch.int64)
        want = minlen(ids, decay(ids, proc(ids, rows[0][None].clone())))[0]
        got = shape_oracle.transform(rows[0], prompt + n, eos=eos, min_new=2, decay=(3, 1.3), start=prompt, pairs=pairs)
        assert _same_bits(got, want), n


def test_thresholds_by_hand():
    row = torch.tensor([1.0, -2.0, 0.0, 4.0])
    E = [1, 2]
    off = shape_oracle.eos_rules(row, 10, E, min_new=3, decay=(5, 2.0), start=7)        # n = 3: neither rule
    assert _same_bits(off, row)
    assert shape_oracle.eos_rules(row, 9, E, min_new=3, decay=(5, 2.0), start=7).tolist() == [1.0, -math.inf, -math.inf, 4.0]     # n = 2 < 3
    assert _same_bits(shape_oracle.eos_rules(row, 12, E, min_new=3, decay=(5, 2.0), start=7), row)        # n = decay_start: not yet
    z = shape_oracle.eos_rules(row, 13, E, min_new=3, decay=(5, 2.0), start=7)          # k = 1: m = 1: z + |z|
    assert z.tolist() == [1.0, 0.0, 0.0, 4.0]
    z = shape_oracle.eos_rules(row, 15, E, min_new=3, decay=(5, 2.0), start=7)          # k = 3: m = 7
    assert z.tolist() == [1.0, -2.0 + 14.0, 0.0, 4.0]
    assert _same_bits(shape_oracle.eos_rules(row, 99, [-1, 4, 1000], min_new=200, decay=None), row)      # no valid EOS id: nothing
    # greedy over the transformed row; the suppression list wins over a decayed EOS
    assert shape_oracle.greedy(row, 15, eos=E, decay=(5, 2.0), start=7) == 1
    assert shape_oracle.greedy(row, 15, eos=E, decay=(5, 2.0), start=7, bad=[1]) == 3


def test_decay_table_saturates_at_2_100():
    assert _bits(shape_oracle.decay_m(2.0, 0)) == 0 and shape_oracle.decay_m(2.0, 1) == 1.0 and shape_oracle.decay_m(2.0, 10) == 1023.0
    assert _bits(shape_oracle.decay_m(2.0, 24)) == _bits(np.float32(2.0 ** 24 - 1))
    assert shape_oracle.decay_m(2.0, 99) == np.float32(2.0 ** 99)
    for k in (100, 101, 127, 128, 1023, 1024, 5000):          # at the clamp, past float32's range, past float64's (pow overflows)
        assert _bits(shape_oracle.decay_m(2.0, k)) == _bits(2.0 ** 100) == 0x71800000, k
    assert _bits(shape_oracle.decay_m(0.9, 5000)) == _bits(-1.0)          # a factor below 1 tends to -1
    assert _bits(shape_oracle.decay_m(1.0, 77)) == 0
    # the decayed logit stays finite there, where HF's is inf
    z = shape_oracle.eos_rules(torch.tensor([3.0, -3.0]), 400, [0, 1], decay=(0, 2.0))
    assert torch.isfinite(z).all() and _bits(z[0]) == _bits(np.float32(3.0) * np.float32(2.0 ** 100)) and z[1] == z[0]


# ------------------------------------------------------------------------------------------ generate()'s gate
class ShapeDevice(ScriptedDevice):
    """the scripted device + a record of every sampling call: ("plain", slot), ("len", slot, min_new, decay, start, eos) and
    ("bias", slot, pairs)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def set_sampling(self, *a, slot=None, **kw):
        self.calls.append(("plain", slot))
        super().set_sampling(*a, slot=slot, **kw)

    def set_length_control(self, min_new_tokens=0, decay=None, start=0, eos_ids=(), slot=None):
        self.calls.append(("len", slot, int(min_new_tokens), (int(decay[0]), round(float(decay[1]), 6)) if decay else None, int(start),
                           tuple(eos_ids)))

    def set_logit_bias(self, logit_bias=None, slot=None):
        self.calls.append(("bias", slot, tuple((int(t), round(float(v), 6)) for t, v in dict(logit_bias or ()).items())))


def test_generate_takes_the_arguments_and_refuses_bad_values():
    dev, proc = ShapeDevice(), fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0)
    T = int(ids.numel())
    kw = dict(input_ids=ids[None], pixel_values=px, bad_words_ids=[[IMG]], max_new_tokens=4, do_sample=True, seed=5)
    plain = dev.generate(**kw)
    assert dev.calls == [("plain", None)]
    dev.calls.clear()
    assert torch.equal(dev.generate(min_new_tokens=5, **kw), plain)          # (the toy LM ignores the sampler's parameters)
    assert dev.calls == [("plain", None), ("len", None, 5, None, T, (EOS,))]      # length_start: the prompt length; E: the config's EOS
    dev.calls.clear()
    assert torch.equal(dev.generate(logit_bias={7: 2.5, "9": -1, 11: 0.0}, **kw), plain)
    assert dev.calls == [("plain", None), ("bias", None, ((7, 2.5), (9, -1.0)))]          # (a bias of 0 is no entry)
    dev.calls.clear()
    dev.generate(min_new_tokens=2, exponential_decay_length_penalty=(3, 1.3), length_start=4, eos_token_id=[EOS, 9],
                 sequence_bias={(7,): 2.5}, logit_bias={8: 1.0}, do_sample=False, **{k: v for k, v in kw.items() if k != "do_sample"})
    assert dev.calls == [("plain", None), ("len", None, 2, (3, 1.3), 4, (EOS, 9)), ("bias", None, ((7, 2.5), (8, 1.0)))]      # greedy too
    dev.calls.clear()
    dev.generate(sequence_bias=[[[7], 2.5], [[3], -4.0]], **kw)              # HF's list form
    assert dev.calls == [("plain", None), ("bias", None, ((3, -4.0), (7, 2.5)))]
    dev.calls.clear()
    # neutral values decode as before, with no call; so does a rule without a valid EOS id
    for neutral in (dict(min_new_tokens=0), dict(min_new_tokens=None), dict(exponential_decay_length_penalty=None), dict(sequence_bias=None),
                    dict(logit_bias=None), dict(logit_bias={}), dict(length_start=3), dict(min_new_tokens=5, eos_token_id=-1),
                    dict(exponential_decay_length_penalty=(1, 2.0), eos_token_id=-1)):
        assert torch.equal(dev.generate(**neutral, **kw)[:, :T + 1], plain[:, :T + 1])
    assert dev.calls == [("plain", None)] * 9
    dev.generation_config.min_new_tokens = 3              # a checkpoint's generation_config.json is honoured
    dev.generation_config.exponential_decay_length_penalty = (6, 1.5)
    dev.calls.clear()
    dev.generate(**kw)
    assert dev.calls == [("plain", None), ("len", None, 3, (6, 1.5), T, (EOS,))]
    dev.generation_config.min_new_tokens = None
    dev.generation_config.exponential_decay_length_penalty = None
    dev.calls.clear()
    bad_values = (
        ("min_new_tokens", dict(min_new_tokens=-1)), ("min_new_tokens", dict(min_new_tokens=1.5)), ("min_new_tokens", dict(min_new_tokens=True)),
        ("exponential_decay_length_penalty", dict(exponential_decay_length_penalty=(1,))),
        ("exponential_decay_length_penalty", dict(exponential_decay_length_penalty=3)),
        ("exponential_decay_length_penalty", dict(exponential_decay_length_penalty=(-1, 1.3))),
        ("exponential_decay_length_penalty", dict(exponential_decay_length_penalty=(1.5, 1.3))),
        ("exponential_decay_length_penalty", dict(exponential_decay_length_penalty=(1, 0.0))),
        ("exponential_decay_length_penalty", dict(exponential_decay_length_penalty=(1, -2.0))),
        ("exponential_decay_length_penalty", dict(exponential_decay_length_penalty=(1, float("nan")))),
        ("exponential_decay_length_penalty", dict(exponential_decay_length_penalty=(1, float("inf")))),
        ("exponential_decay_length_penalty", dict(exponential_decay_length_penalty=(1, "2"))),
        ("min_new_tokens", dict(min_new_tokens=5, exponential_decay_length_penalty=(4, 1.3))),          # the decay would start below the minimum
        ("length_start", dict(min_new_tokens=2, length_start=-1)), ("length_start", dict(min_new_tokens=2, length_start=1.5)),
        ("logit_bias", dict(logit_bias={-1: 1.0})), ("logit_bias", dict(logit_bias={VOCAB: 1.0})), ("logit_bias", dict(logit_bias={1.5: 1.0})),
        ("logit_bias", dict(logit_bias={7: 100.5})), ("logit_bias", dict(logit_bias={7: -101})), ("logit_bias", dict(logit_bias={7: float("nan")})),
        ("logit_bias", dict(logit_bias={7: float("inf")})), ("logit_bias", dict(logit_bias={7: "1"})), ("logit_bias", dict(logit_bias=[(7, 1.0)])),
        ("at most 256", dict(logit_bias={t: 1.0 for t in range(3, 260)})),
        ("sequence_bias", dict(sequence_bias={})), ("sequence_bias", dict(sequence_bias={(): 1.0})), ("sequence_bias", dict(sequence_bias={(-3,): 1.0})),
        ("sequence_bias", dict(sequence_bias={(7,): 200.0})), ("sequence_bias", dict(sequence_bias="ab")),
        ("biased twice", dict(sequence_bias={(7,): 1.0}, logit_bias={7: 2.0})),
        ("at most 8", dict(min_new_tokens=2, eos_token_id=list(range(3, 12)))),
    )
    for match, bad in bad_values:
        with pytest.raises(ValueError, match=match):
            dev.generate(**bad, **kw)
    with pytest.raises(NotImplementedError, match="multi-token"):
        dev.generate(sequence_bias={(7, 8): 1.0}, **kw)
    assert dev.calls == []                                      # ... before anything runs
    assert check_length_control() == (0, None, None) and check_length_control(4, (4, 2), 0) == (4, (4, 2.0), 0)
    assert check_logit_bias() == () and check_logit_bias({t: -100 for t in range(256)}, None, 256) == tuple((t, -100.0) for t in range(256))
    # what stays refused stays refused
    for refused in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=3), dict(min_length=4), dict(typical_p=0.5), dict(eta_cutoff=0.1),
                    dict(num_beams=2), dict(num_return_sequences=2), dict(penalty_alpha=0.5)):
        with pytest.raises(NotImplementedError):
            dev.generate(min_new_tokens=2, **refused, **kw)
    # the plain scripted device (no such call on its "library") still decodes, and says so when asked for a value
    old = ScriptedDevice()
    assert torch.equal(old.generate(**kw), plain)
    with pytest.raises(_lib.DtkError, match="length control"):
        old.generate(min_new_tokens=2, **kw)
    with pytest.raises(_lib.DtkError, match="logit bias"):
        old.generate(logit_bias={7: 1.0}, **kw)


def test_generator_counts_from_the_end_of_its_prompt():
    """DetikzifyGenerator(min_new_tokens=...): a rollout that continues a node carries length_start = the length of the image prompt"""
    from detikzify_amd.infer import DetikzifyGenerator
    from .helpers import sketch_image
    dev, proc = ShapeDevice(), fake_processor(VOCAB, NIMG)
    gen = DetikzifyGenerator(dev, proc, sketch_image(0, 32), min_new_tokens=6, exponential_decay_length_penalty=(40, 1.1), logit_bias={9: -2.0},
                             max_length=60, do_sample=True, temperature=1.0, top_p=1.0, top_k=0, metric=None)
    root = gen.montecarlo.root_node.token_ids
    eos = int(proc.tokenizer.eos_token_id)
    node = torch.cat([root, torch.tensor([7, 8, 9], dtype=torch.int64)])
    gen.generate(node)
    want_eos = tuple(sorted({EOS}))
    assert dev.calls == [("plain", None), ("len", None, 6, (40, 1.1), int(root.numel()), want_eos), ("bias", None, ((9, -2.0),))]
    dev.calls.clear()
    gen.generate(root, length_start=0)
    assert dev.calls == [("plain", None), ("len", None, 6, (40, 1.1), 0, want_eos), ("bias", None, ((9, -2.0),))]
    assert eos >= 0


# ------------------------------------------------------------------------------------------ the C ABI
NEW = {
    "dtk_set_length_control": "(dtk_ctx* ctx, const dtk_length_ctl* l)",
    "dtk_set_length_control_slot": "(dtk_ctx* ctx, int slot, const dtk_length_ctl* l)",
    "dtk_set_logit_bias": "(dtk_ctx* ctx, const int32_t* ids, const float* values, int n)",
    "dtk_set_logit_bias_slot": "(dtk_ctx* ctx, int slot, const int32_t* ids, const float* values, int n)",
    "dtk_logit_bias_table": "(dtk_ctx* ctx, int slot, float* out, int V)",
    "dtk_op_sample_shape": "(dtk_ctx* ctx, const float* logits, int V, int step, int64_t* token_out, float* filtered_probs_out, "
                           "float* lp_out /* [2] or NULL */, const dtk_sampling_ext* x /* or NULL */, float presence, float frequency, "
                           "const int64_t* counted_ids, int n_counted, const int64_t* history, int n_history, const dtk_dry* d, "
                           "int cur, const dtk_length_ctl* l, const int32_t* bias_ids, const float* bias_values, int n_bias)",
    "dtk_engine_submit_shape": "(dtk_engine* e, dtk_join* j, const dtk_sampling_ext* x /* or NULL */, float presence, float frequency, int start, "
                               "const dtk_dry* d /* or NULL */, const dtk_length_ctl* l /* or NULL */, const int32_t* bias_ids, "
                               "const float* bias_values, int n_bias, const int64_t* text_ids, int n_text, uint64_t text_key, "
                               "uint64_t* ticket_out)",
    "dtk_engine_set_length_control_op": "(dtk_engine* e, int (*set_length_control_slot)(void* dev, int slot, const dtk_length_ctl* l))",
    "dtk_engine_set_logit_bias_op": "(dtk_engine* e, int (*set_logit_bias_slot)(void* dev, int slot, const int32_t* ids, const float* values, int n))",
}


def test_abi_is_additive_and_bound():
    assert _lib.DTK_ABI_VERSION == 7 and re.search(r"#define DTK_ABI_VERSION 7\b", HEADER)
    assert re.search(r"#define DTK_BIAS_MAX 256\b", HEADER) and _lib.DTK_BIAS_MAX == 256 == shape_oracle.BIAS_MAX and _lib.DTK_LEN_MAX_EOS == 8
    flat = re.sub(r"\s+", " ", HEADER)
    X, F, I32, I64, U64 = C.POINTER(_lib.DtkSamplingExt), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    P, I, FL, D, L = C.c_void_p, C.c_int, C.c_float, C.POINTER(_lib.DtkDry), C.POINTER(_lib.DtkLengthCtl)
    bound = {       # the header's parameter lists above, as ctypes (pointers to anything else: void*)
        "dtk_set_length_control": [P, L],
        "dtk_set_length_control_slot": [P, I, L],
        "dtk_set_logit_bias": [P, I32, F, I],
        "dtk_set_logit_bias_slot": [P, I, I32, F, I],
        "dtk_logit_bias_table": [P, I, F, I],
        "dtk_op_sample_shape": [P, P, I, I, I64, P, F, X, FL, FL, I64, I, I64, I, D, I, L, I32, F, I],
        "dtk_engine_submit_shape": [P, C.POINTER(_lib.DtkJoin), X, FL, FL, I, D, L, I32, F, I, I64, I, C.c_uint64, U64],
        "dtk_engine_set_length_control_op": [P, _lib.DtkEngineOps.LENGTH_CTL],
        "dtk_engine_set_logit_bias_op": [P, _lib.DtkEngineOps.LOGIT_BIAS],
    }
    for name, params in NEW.items():
        assert f"int {name}{params};" in flat.replace("int  ", "int "), name
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and list(args) == bound[name], name
    # dtk_op_sample_shape is dtk_op_sample_dry's signature plus cur, the struct and the pairs; the submit variant likewise
    assert list(_lib.SYMBOLS["dtk_op_sample_shape"][1][:-5]) == list(_lib.SYMBOLS["dtk_op_sample_dry"][1])
    dry_submit = list(_lib.SYMBOLS["dtk_engine_submit_dry"][1])
    assert list(_lib.SYMBOLS["dtk_engine_submit_shape"][1]) == dry_submit[:7] + [L, I32, F, I] + dry_submit[7:]
    assert _lib.DtkEngineOps.LENGTH_CTL._argtypes_ == (C.c_void_p, C.c_int, L)
    assert _lib.DtkEngineOps.LOGIT_BIAS._argtypes_ == (C.c_void_p, C.c_int, I32, F, C.c_int)
    # the struct as the header lays it out
    m = re.search(r"typedef struct dtk_length_ctl \{(.*?)\} dtk_length_ctl;", HEADER, re.S)
    fields = [re.sub(r"\[.*", "", f.split()[-1]) for f in m.group(1).split(";") if f.strip()]
    assert fields == [n for n, _ in _lib.DtkLengthCtl._fields_]
    lib = _lib.load_library()
    assert lib.dtk_abi_version() == 7
    assert lib.dtk_abi_struct_size(16) == C.sizeof(_lib.DtkLengthCtl) == 56
    # the pinned layouts did not move
    assert lib.dtk_abi_struct_size(14) == C.sizeof(_lib.DtkDry) == 84
    assert lib.dtk_abi_struct_size(12) == C.sizeof(_lib.DtkSamplingExt) == 32
    assert lib.dtk_abi_struct_size(1) == C.sizeof(_lib.DtkSampling) == 136
    assert lib.dtk_abi_struct_size(6) == C.sizeof(_lib.DtkJoin)
    assert lib.dtk_abi_struct_size(13) == -1 and lib.dtk_abi_struct_size(15) == -1 and lib.dtk_abi_struct_size(17) == -1
    # null contexts / engines are an error code, not a crash
    l, d, tok, t = _lib.DtkLengthCtl(2, 0, 0.0, 0, 1), _lib.DtkDry(0.0, 1.75, 2, 0, 0), C.c_int64(), C.c_uint64()
    ids, vals, logits = (C.c_int32 * 4)(), (C.c_float * 4)(), (C.c_float * 4)()
    assert lib.dtk_set_length_control(None, C.byref(l)) == -1 and lib.dtk_set_length_control_slot(None, 0, C.byref(l)) == -1
    assert lib.dtk_set_logit_bias(None, ids, vals, 1) == -1 and lib.dtk_set_logit_bias_slot(None, 0, ids, vals, 1) == -1
    assert lib.dtk_logit_bias_table(None, -1, logits, 4) == -1
    assert lib.dtk_op_sample_shape(None, C.cast(logits, C.c_void_p), 4, 0, C.byref(tok), None, None, None, 0.0, 0.0, None, 0, None, 0,
                                   C.byref(d), 3, C.byref(l), ids, vals, 1) == -1
    assert lib.dtk_engine_submit_shape(None, C.byref(_lib.DtkJoin()), None, 0.0, 0.0, 0, C.byref(d), C.byref(l), ids, vals, 1, None, 0, 0,
                                       C.byref(t)) == -1
    assert lib.dtk_engine_set_length_control_op(None, _lib.DtkEngineOps.LENGTH_CTL()) == -1
    assert lib.dtk_engine_set_logit_bias_op(None, _lib.DtkEngineOps.LOGIT_BIAS()) == -1


# ------------------------------------------------------------------------------------------ both engines
@pytest.mark.parametrize("engine", [NativeBatchEngine, BatchEngine], ids=["native", "python"])
def test_engines_carry_the_values_with_the_join_and_reset_them(engine):
    proc = fake_processor(VOCAB, NIMG)
    dev = ShapeDevice(slots=5)
    eng = engine(dev, max_batch=1, share_prefix=False)           # one decoding slot: every sequence takes slot 0
    try:
        ids, px = _prompt(proc, 1)
        T = int(ids.numel())
        kw = dict(input_ids=ids[None], pixel_values=px, bad_words_ids=[[IMG]], max_new_tokens=5, do_sample=True)
        a = dev.generate(seed=1, min_new_tokens=5, eos_token_id=[EOS], **kw)
        b = dev.generate(seed=2, eos_token_id=-1, **kw)
        c = dev.generate(seed=3, min_new_tokens=1, exponential_decay_length_penalty=(2, 1.5), length_start=2, logit_bias={7: 1.5, 300: -3.0},
                         eos_token_id=[EOS, 11], **kw)
        d = dev.generate(seed=4, sequence_bias={(5,): 0.25}, eos_token_id=-1, **kw)
    finally:
        eng.close()
    assert b.shape[1] == d.shape[1] == T + 5 and a.shape[1] <= T + 5 and c.shape[1] <= T + 5
    per_join = [[x for x in dev.calls[i:] if x[0] != "plain"][:2] for i, x in enumerate(dev.calls) if x[0] == "plain"]
    assert len(per_join) == 4 and all(x[1] == 0 for x in dev.calls)
    # every join sets (or resets) both records, after the plain call
    assert per_join[0] == [("len", 0, 5, None, T, (EOS,)), ("bias", 0, ())]
    assert per_join[1] == [("len", 0, 0, None, 0, ()), ("bias", 0, ())]
    assert per_join[2] == [("len", 0, 1, (2, 1.5), 2, (EOS, 11)), ("bias", 0, ((7, 1.5), (300, -3.0)))]
    assert per_join[3] == [("len", 0, 0, None, 0, ()), ("bias", 0, ((5, 0.25),))]
    # out of range never reaches the device
    dev2 = ShapeDevice(slots=5)
    eng = engine(dev2, max_batch=1, share_prefix=False)
    try:
        for bad, match in ((dict(min_new_tokens=-2), "min_new_tokens"), (dict(exponential_decay_length_penalty=(0, 0.0)), "decay_factor"),
                           (dict(logit_bias={7: 1000.0}), "logit_bias")):
            with pytest.raises(ValueError, match=match):
                with eng.sequence(ids, px, dict(do_sample=True, length_eos_ids=(EOS,), **bad)):
                    pass
        assert dev2.calls == []
    finally:
        eng.close()


def test_native_engine_without_the_ops_refuses_a_join_with_values():
    """an engine of dtk_engine_create_ops that has no length / bias op: a join with values fails in submit, one without joins"""
    proc = fake_processor(VOCAB, NIMG)
    dev = ScriptedDevice(slots=5)
    eng = NativeBatchEngine(dev, max_batch=2, share_prefix=False)
    lib = _lib.load_library()
    try:
        assert lib.dtk_engine_set_length_control_op(eng._h, _lib.DtkEngineOps.LENGTH_CTL()) == 0       # take the ops away again
        assert lib.dtk_engine_set_logit_bias_op(eng._h, _lib.DtkEngineOps.LOGIT_BIAS()) == 0
        ids, px = _prompt(proc, 2)
        with pytest.raises(_lib.DtkError, match="dtk_engine_set_length_control_op"):
            with eng.sequence(ids, px, dict(do_sample=True, seed=3, min_new_tokens=2, length_eos_ids=(EOS,)), max_new_tokens=3):
                pass
        with pytest.raises(_lib.DtkError, match="dtk_engine_set_logit_bias_op"):
            with eng.sequence(ids, px, dict(do_sample=True, seed=3, logit_bias=((7, 1.0),)), max_new_tokens=3):
                pass
        out = dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=3, do_sample=True, seed=3, eos_token_id=-1)
        assert out.shape[1] == ids.numel() + 3
        j, t = _lib.DtkJoin(), C.c_uint64()
        L = _lib.DtkLengthCtl
        for bad in (L(-1, 0, 0.0, 0, 0), L(0, -1, 0.0, 0, 0), L(0, 0, -1.0, 0, 0), L(0, 0, float("nan"), 0, 0), L(0, 0, float("inf"), 0, 0),
                    L(3, 2, 1.5, 0, 0), L(0, 0, 0.0, -1, 0), L(0, 0, 0.0, 0, 9)):
            assert lib.dtk_engine_submit_shape(eng._h, C.byref(j), None, 0.0, 0.0, 0, None, C.byref(bad), None, None, 0, None, 0, 0, C.byref(t)) == -1
            assert b"min_new_tokens" in j.error_out
        one, big = (C.c_int32 * 1)(7), (C.c_float * 1)(100.5)
        assert lib.dtk_engine_submit_shape(eng._h, C.byref(j), None, 0.0, 0.0, 0, None, None, one, big, 1, None, 0, 0, C.byref(t)) == -1
        assert lib.dtk_engine_submit_shape(eng._h, C.byref(j), None, 0.0, 0.0, 0, None, None, one, big, 257, None, 0, 0, C.byref(t)) == -1
        assert b"bias" in j.error_out
    finally:
        eng.close()
