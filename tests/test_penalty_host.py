"""presence_penalty / frequency_penalty without a GPU: the specification (tests/penalty_oracle.py) on hand cases with the exact float32 bits,
generate()'s argument gate, the additive C ABI, and the penalties call of both batch engines over the scripted device."""
from __future__ import annotations

import ctypes as C
import re
import struct
from pathlib import Path

import pytest
import torch

from detikzify_amd import _lib
from detikzify_amd.infer.batching import BatchEngine
from detikzify_amd.infer.engine import NativeBatchEngine
from oracle import sampling

from . import penalty_oracle
from .helpers import fake_processor
from .test_generate_loop import IMG, NIMG, VOCAB, ScriptedDevice, _prompt

HEADER = (Path(__file__).resolve().parents[1] / "include" / "dtk.h").read_text()


def _bits(x) -> int:
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


# ------------------------------------------------------------------------------------------ exact bits
def test_hand_cases_with_exact_float32_bits():
    row = torch.tensor([1.0, 1.0, 0.5, 2.0, 2.0, -1.25, float("-inf"), 3.0])
    before = [_bits(v) for v in row]
    # a count of 1: pen = f32(f64(f32(.6)) + f64(f32(.4))) = 1.0 exactly; of 3: f32(.6 + .4 * 3) = 0x3fe66667
    z = penalty_oracle.penalise(row, [0], 0.6, 0.4)
    assert _bits(z[0]) == 0x00000000 and [_bits(v) for v in z[1:]] == before[1:]          # every untouched id keeps its bits
    z = penalty_oracle.penalise(row, [1, 1, 1], 0.6, 0.4)
    assert _bits(z[1]) == 0xBF4CCCCE and _bits(z[0]) == before[0]
    # negative values raise a counted logit: 0.5 - (-0.5 - 0.25 * 2) = 1.5
    z = penalty_oracle.penalise(row, [2, 2], -0.5, -0.25)
    assert _bits(z[2]) == 0x3FC00000
    # presence only (the count does not matter) and frequency only (it does): 2 - f32(.3) = 2 - f32(f64(f32(.1)) * 3) = 0x3fd9999a
    z = penalty_oracle.penalise(row, [3] * 5, 0.3, 0.0)
    assert _bits(z[3]) == 0x3FD9999A
    z = penalty_oracle.penalise(row, [4] * 3, 0.0, 0.1)
    assert _bits(z[4]) == 0x3FD9999A
    z = penalty_oracle.penalise(row, [4], 0.0, 0.1)
    assert _bits(z[4]) == _bits(torch.tensor(2.0) - torch.tensor(0.1))
    # a count of 7: -1.25 - f32(.6 + .4 * 7) = -1.25 - 0x4059999a
    z = penalty_oracle.penalise(row, [5] * 7, 0.6, 0.4)
    assert _bits(z[5]) == 0xC094CCCD
    # -inf stays -inf (a logit that is -inf already), and a banned id that is also counted stays -inf behind the suppression list
    z = penalty_oracle.penalise(row, [6, 6], -2.0, -2.0)
    assert _bits(z[6]) == 0xFF800000
    z = penalty_oracle.penalise(row, [7, 7], -2.0, -2.0)             # 3 + 6 = 9: the arg-max by far, but banned
    assert float(z[7]) == 9.0
    assert penalty_oracle.greedy(row, [7, 7], -2.0, -2.0, bad=[7]) == 3            # 2.0 twice: the lowest id
    tok, probs, _ = penalty_oracle.draw(row, [7, 7], -2.0, -2.0, 1.0, 0, 1.0, seed=1, n=0, bad=[7])
    assert float(probs[7]) == 0.0 and tok != 7
    # the penalty moves the arg-max; off is the plain oracle, bit for bit
    assert sampling.greedy(row) == 7 and penalty_oracle.greedy(row, [7], 1.5, 0.0) == 3
    assert torch.equal(penalty_oracle.penalise(row, [0, 3, 7], 0.0, 0.0)[:6], row[:6])
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(1000, generator=g) * 3
    for n in range(8):
        t0, p0 = sampling.draw(logits, 0.9, 50, 0.9, 77, n, [1], [2], n == 0)
        t1, p1, _ = penalty_oracle.draw(logits, [5, 5, 9], 0.0, 0.0, 0.9, 50, 0.9, 77, n, bad=[1], begin=[2], first=n == 0)
        assert t0 == t1 and torch.equal(p0, p1)


# ------------------------------------------------------------------------------------------ generate()'s gate
class PenDevice(ScriptedDevice):
    """the scripted device + a record of every sampling call: ("plain", slot) and ("pen", slot, presence, frequency, start)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def set_sampling(self, *a, slot=None, **kw):
        self.calls.append(("plain", slot))
        super().set_sampling(*a, slot=slot, **kw)

    def set_penalties(self, presence=0.0, frequency=0.0, start=0, slot=None):
        self.calls.append(("pen", slot, round(float(presence), 6), round(float(frequency), 6), int(start)))


def test_generate_takes_the_penalties_and_still_refuses_the_rest():
    dev, proc = PenDevice(), fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0)
    T = int(ids.numel())
    kw = dict(input_ids=ids[None], pixel_values=px, bad_words_ids=[[IMG]], max_new_tokens=4, do_sample=True, seed=5)
    plain = dev.generate(**kw)
    assert dev.calls == [("plain", None)]
    dev.calls.clear()
    assert torch.equal(dev.generate(presence_penalty=0.6, frequency_penalty=0.4, **kw), plain)      # (the toy LM ignores the sampler's parameters)
    assert dev.calls == [("plain", None), ("pen", None, 0.6, 0.4, T)]                              # penalty_start: the prompt length
    dev.calls.clear()
    dev.generate(frequency_penalty=-0.5, penalty_start=3, do_sample=False, **{k: v for k, v in kw.items() if k != "do_sample"})
    assert dev.calls == [("plain", None), ("pen", None, 0.0, -0.5, 3)]                              # greedy takes them as well
    dev.calls.clear()
    dev.generate(presence_penalty=0.0, frequency_penalty=0.0, **kw)        # off: no call
    dev.generate(presence_penalty=None, frequency_penalty=None, penalty_start=7, **kw)
    assert dev.calls == [("plain", None)] * 2
    dev.generation_config.presence_penalty = 0.25                          # a checkpoint's generation_config.json is honoured
    dev.calls.clear()
    dev.generate(**kw)
    assert dev.calls == [("plain", None), ("pen", None, 0.25, 0.0, T)]
    del dev.generation_config.presence_penalty
    dev.calls.clear()
    for name in ("presence_penalty", "frequency_penalty"):
        for bad in (-2.5, 2.0001, float("nan"), float("inf"), "1"):
            with pytest.raises(ValueError, match=re.escape(f"`{name}` has to be a float in the [-2, 2] interval")):
                dev.generate(**{name: bad}, **kw)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="penalty_start"):
            dev.generate(presence_penalty=0.5, penalty_start=bad, **kw)
    assert dev.calls == []                                                 # ... before anything runs
    with pytest.raises(NotImplementedError):
        dev.generate(repetition_penalty=1.2, **kw)
    with pytest.raises(NotImplementedError):
        dev.generate(typical_p=0.9, **kw)
    with pytest.raises(NotImplementedError):
        dev.generate(no_repeat_ngram_size=3, **kw)
    assert dev.generate(repetition_penalty=1.0, **kw).shape == plain.shape
    # the plain scripted device (no such call on its "library") still decodes, and says so when asked for a value
    old = ScriptedDevice()
    assert torch.equal(old.generate(**kw), plain)
    with pytest.raises(_lib.DtkError, match="penalty"):
        old.generate(presence_penalty=0.1, **kw)


def test_generator_counts_from_the_end_of_its_prompt():
    """DetikzifyGenerator(presence_penalty=, frequency_penalty=): a rollout that continues a node carries penalty_start = the length of
    the image prompt, not of the node's ids"""
    from detikzify_amd.infer import DetikzifyGenerator
    from .helpers import sketch_image
    dev, proc = PenDevice(), fake_processor(VOCAB, NIMG)
    gen = DetikzifyGenerator(dev, proc, sketch_image(0, 32), presence_penalty=0.5, frequency_penalty=0.25, max_length=60, do_sample=True,
                             temperature=1.0, top_p=1.0, top_k=0, metric=None)
    root = gen.montecarlo.root_node.token_ids
    node = torch.cat([root, torch.tensor([7, 8, 9], dtype=torch.int64)])
    gen.generate(node)
    assert dev.calls == [("plain", None), ("pen", None, 0.5, 0.25, int(root.numel()))]
    dev.calls.clear()
    gen.generate(root, penalty_start=0)
    assert dev.calls == [("plain", None), ("pen", None, 0.5, 0.25, 0)]


# ------------------------------------------------------------------------------------------ the C ABI
NEW = {
    "dtk_set_penalties": "(dtk_ctx* ctx, float presence, float frequency, int start)",
    "dtk_set_penalties_slot": "(dtk_ctx* ctx, int slot, float presence, float frequency, int start)",
    "dtk_op_sample_pen": "(dtk_ctx* ctx, const float* logits, int V, int step, int64_t* token_out, float* filtered_probs_out, "
                         "float* lp_out /* [2] or NULL */, const dtk_sampling_ext* x /* or NULL */, float presence, float frequency, "
                         "const int64_t* counted_ids, int n_counted)",
    "dtk_token_counts": "(dtk_ctx* ctx, int slot, uint16_t* out, int V)",
    "dtk_engine_submit_pen": "(dtk_engine* e, dtk_join* j, const dtk_sampling_ext* x /* or NULL */, float presence, float frequency, int start, "
                             "const int64_t* text_ids, int n_text, uint64_t text_key, uint64_t* ticket_out)",
    "dtk_engine_set_penalties_op": "(dtk_engine* e, int (*set_penalties_slot)(void* dev, int slot, float presence, float frequency, int start))",
}


def test_abi_is_additive_and_bound():
    assert _lib.DTK_ABI_VERSION == 7 and re.search(r"#define DTK_ABI_VERSION 7\b", HEADER)
    flat = re.sub(r"\s+", " ", HEADER)
    X, F, I64, U64 = C.POINTER(_lib.DtkSamplingExt), C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    P, I, FL = C.c_void_p, C.c_int, C.c_float
    bound = {       # the header's parameter lists above, as ctypes (pointers to anything else: void*)
        "dtk_set_penalties": [P, FL, FL, I],
        "dtk_set_penalties_slot": [P, I, FL, FL, I],
        "dtk_op_sample_pen": [P, P, I, I, I64, P, F, X, FL, FL, I64, I],
        "dtk_token_counts": [P, I, C.POINTER(C.c_uint16), I],
        "dtk_engine_submit_pen": [P, C.POINTER(_lib.DtkJoin), X, FL, FL, I, I64, I, C.c_uint64, U64],
        "dtk_engine_set_penalties_op": [P, _lib.DtkEngineOps.PENALTIES],
    }
    for name, params in NEW.items():
        assert f"int {name}{params};" in flat.replace("int  ", "int "), name
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and list(args) == bound[name], name
    # dtk_op_sample_pen is dtk_op_sample_ext's signature plus the two values and the token list
    assert list(_lib.SYMBOLS["dtk_op_sample_pen"][1][:-4]) == list(_lib.SYMBOLS["dtk_op_sample_ext"][1])
    assert _lib.DtkEngineOps.PENALTIES._argtypes_ == (C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int)
    lib = _lib.load_library()
    assert lib.dtk_abi_version() == 7
    # the pinned layouts did not move, and no struct was added
    assert lib.dtk_abi_struct_size(12) == C.sizeof(_lib.DtkSamplingExt) == 32
    assert lib.dtk_abi_struct_size(1) == C.sizeof(_lib.DtkSampling) == 136
    assert lib.dtk_abi_struct_size(6) == C.sizeof(_lib.DtkJoin)
    assert lib.dtk_abi_struct_size(13) == -1
    # null contexts / engines are an error code, not a crash
    buf, tok, t = (C.c_uint16 * 4)(), C.c_int64(), C.c_uint64()
    logits = (C.c_float * 4)()
    assert lib.dtk_set_penalties(None, 0.5, 0.5, 0) == -1 and lib.dtk_set_penalties_slot(None, 0, 0.5, 0.5, 0) == -1
    assert lib.dtk_token_counts(None, -1, buf, 4) == -1
    assert lib.dtk_op_sample_pen(None, C.cast(logits, C.c_void_p), 4, 0, C.byref(tok), None, None, None, 0.5, 0.5, None, 0) == -1
    assert lib.dtk_engine_submit_pen(None, C.byref(_lib.DtkJoin()), None, 0.5, 0.5, 0, None, 0, 0, C.byref(t)) == -1
    assert lib.dtk_engine_set_penalties_op(None, _lib.DtkEngineOps.PENALTIES()) == -1


# ------------------------------------------------------------------------------------------ both engines
@pytest.mark.parametrize("engine", [NativeBatchEngine, BatchEngine], ids=["native", "python"])
def test_engines_carry_the_values_with_the_join_and_reset_them(engine):
    proc = fake_processor(VOCAB, NIMG)
    dev = PenDevice(slots=5)
    eng = engine(dev, max_batch=1, share_prefix=False)           # one decoding slot: every sequence takes slot 0
    try:
        ids, px = _prompt(proc, 1)
        T = int(ids.numel())
        kw = dict(input_ids=ids[None], pixel_values=px, bad_words_ids=[[IMG]], max_new_tokens=5, do_sample=True, eos_token_id=-1)
        a = dev.generate(seed=1, presence_penalty=0.6, frequency_penalty=0.4, **kw)
        b = dev.generate(seed=2, **kw)
        c = dev.generate(seed=3, frequency_penalty=-1.0, penalty_start=2, **kw)
    finally:
        eng.close()
    assert a.shape[1] == b.shape[1] == c.shape[1] == T + 5
    assert dev.calls == [("plain", 0), ("pen", 0, 0.6, 0.4, T), ("plain", 0), ("pen", 0, 0.0, 0.0, 0), ("plain", 0), ("pen", 0, 0.0, -1.0, 2)]
    # out of range never reaches the device
    dev2 = PenDevice(slots=5)
    eng = engine(dev2, max_batch=1, share_prefix=False)
    try:
        with pytest.raises(ValueError, match="presence_penalty"):
            with eng.sequence(ids, px, dict(do_sample=True, presence_penalty=2.5)):
                pass
        assert dev2.calls == []
    finally:
        eng.close()


def test_native_engine_without_the_op_refuses_a_join_with_values():
    """an engine of dtk_engine_create_ops that has no penalties op: a join with values fails in submit, one with 0 / 0 joins"""
    proc = fake_processor(VOCAB, NIMG)
    dev = ScriptedDevice(slots=5)
    eng = NativeBatchEngine(dev, max_batch=2, share_prefix=False)
    lib = _lib.load_library()
    try:
        assert lib.dtk_engine_set_penalties_op(eng._h, _lib.DtkEngineOps.PENALTIES()) == 0       # take the op away again
        ids, px = _prompt(proc, 2)
        with pytest.raises(_lib.DtkError, match="dtk_engine_set_penalties_op"):
            with eng.sequence(ids, px, dict(do_sample=True, seed=3, frequency_penalty=0.2), max_new_tokens=3):
                pass
        out = dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=3, do_sample=True, seed=3, eos_token_id=-1)
        assert out.shape[1] == ids.numel() + 3
        j, t = _lib.DtkJoin(), C.c_uint64()
        for pp, fp, st in ((2.5, 0.0, 0), (0.0, float("nan"), 0), (0.5, 0.5, -1)):
            assert lib.dtk_engine_submit_pen(eng._h, C.byref(j), None, pp, fp, st, None, 0, 0, C.byref(t)) == -1 and b"penalty" in j.error_out
    finally:
        eng.close()
