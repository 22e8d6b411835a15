"""DRY without a GPU: the specification (tests/dry_oracle.py) against a brute-force version and on hand cases, the exact float32 bits of
the penalty table, generate()'s argument gate, the additive C ABI, and the DRY call of both batch engines over the scripted device."""
from __future__ import annotations

import ctypes as C
import random
import re
import struct
from pathlib import Path

import pytest
import torch

from detikzify_amd import _lib
from detikzify_amd.infer.batching import BatchEngine
from detikzify_amd.infer.engine import NativeBatchEngine
from detikzify_amd.model.modeling import check_dry

from . import dry_oracle
from .helpers import fake_processor
from .test_generate_loop import IMG, NIMG, VOCAB, ScriptedDevice, _prompt

HEADER = (Path(__file__).resolve().parents[1] / "include" / "dtk.h").read_text()


def _bits(x) -> int:
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


# ------------------------------------------------------------------------------------------ the rule
def _brute(h, B):
    """M by trying every pair (i, L) from the definition: L is valid iff every k in [1, L) passes all three conditions"""
    n, M = len(h), {}
    if n < 2:
        return M
    if h[n - 1] in B:
        return M
    for i in range(0, n - 1):
        if not (h[i] == h[n - 1]):
            continue
        if h[i + 1] in B:
            continue
        best = 0
        for L in range(1, 65):
            ok = True
            for k in range(1, L):
                if i - k < 0:
                    ok = False
                elif h[i - k] != h[n - 1 - k]:
                    ok = False
                elif h[n - 1 - k] in B:
                    ok = False
            if ok and L > best:
                best = L
        t = h[i + 1]
        if t not in M or M[t] < best:
            M[t] = best
    return M


def test_oracle_equals_brute_force_on_seeded_histories():
    rng = random.Random(20260)
    longest = 0
    for case in range(300):
        alphabet = rng.randint(3, 5)
        n = rng.randint(0, 120)
        if case % 3 == 0:       # periodic with a few defects: long matches
            period = [rng.randrange(alphabet) for _ in range(rng.randint(1, 6))]
            h = [period[i % len(period)] for i in range(n)]
            for _ in range(rng.randint(0, 3)):
                if n:
                    h[rng.randrange(n)] = rng.randrange(alphabet)
        else:
            h = [rng.randrange(alphabet) for _ in range(n)]
        B = set(rng.sample(range(alphabet), rng.randint(0, 1))) if case % 2 else set()
        got = dry_oracle.match_lengths(h, B)
        assert got == _brute(h, B), (case, h, B)
        longest = max([longest] + list(got.values()))
    assert longest == 64          # the cap was reached somewhere


def test_hand_cases():
    a, b, c = 10, 11, 12
    assert dry_oracle.match_lengths([a, b, c, a, b]) == {c: 2}
    assert dry_oracle.penalised_ids([a, b, c, a, b], 2) == {c: 2} and dry_oracle.penalised_ids([a, b, c, a, b], 3) == {}
    assert dry_oracle.match_lengths([5] * 10) == {5: 9}                    # period 1: the match overlaps the tail
    assert dry_oracle.match_lengths([5] * 100) == {5: 64}
    assert dry_oracle.match_lengths([a, b, c] * 30) == {a: 64}             # the cap
    assert dry_oracle.match_lengths([a, b, c] * 21) == {a: 60}             # below it: i = 59, L = 60
    assert dry_oracle.match_lengths([a, b, c, a, b, c]) == {a: 3}          # the match runs into position 0
    assert dry_oracle.match_lengths([a, b, c, a, b], [b]) == {}            # a breaker as the last token
    assert dry_oracle.match_lengths([a, b, c, a, b], [c]) == {}            # ... as the next token
    assert dry_oracle.match_lengths([9, a, b, c, 9, a, b]) == {c: 3}
    assert dry_oracle.match_lengths([9, a, b, c, 9, a, b], [a]) == {c: 1}  # ... inside the match: it ends there
    assert dry_oracle.match_lengths([9, a, b, c, 9, a, b], [9]) == {c: 2}
    assert dry_oracle.match_lengths([]) == {} and dry_oracle.match_lengths([3]) == {}
    assert dry_oracle.match_lengths([3, 3]) == {3: 1} and dry_oracle.match_lengths([3, 4]) == {}
    # two continuations of one tail: the longer match wins per id
    assert dry_oracle.match_lengths([a, b, 1, 7, a, b, 2, 7, a, b]) == {1: 2, 2: 3}
    # z': only penalised ids move, by one fp32 subtraction; off is the row itself
    row = torch.tensor([0.5, 1.0, 2.0, 3.0])
    z = dry_oracle.penalise(row, [0, 1, 2, 0, 1], 0.8, 1.75, 2)
    assert _bits(z[2]) == _bits(torch.tensor(2.0) - torch.tensor(0.8)) and [_bits(v) for v in z[[0, 1, 3]]] == [_bits(v) for v in row[[0, 1, 3]]]
    assert torch.equal(dry_oracle.penalise(row, [0, 1, 2, 0, 1], 0.0), row)
    assert dry_oracle.greedy(row, [1, 0, 3, 1, 0], 4.0) == 2 and dry_oracle.greedy(row, [1, 0, 3, 1], 4.0) == 3      # (a match of 1 < allowed_length)
    # with a presence / frequency pair: theirs first, DRY's second
    z = dry_oracle.both(row, [2], 0.6, 0.4, [0, 1, 2, 0, 1], 0.8)
    assert _bits(z[2]) == _bits((torch.tensor(2.0) - torch.tensor(1.0)) - torch.tensor(0.8))


def test_table_bits():
    t = dry_oracle.table(0.8, 1.75, 2)
    assert [_bits(v) for v in t[:8]] == [0, 0, 0x3F4CCCCD, 0x3FB33333, 0x401CCCCD, 0x40893333, 0x40F0199A, 0x41521667]
    assert _bits(t[64]) == 0x5854E819
    t = dry_oracle.table(100.0, 8.0, 1)
    assert [_bits(v) for v in t[:4]] == [0, 0x42C80000, 0x44480000, 0x45C80000]
    assert [_bits(v) for v in t[31:35]] == [0x6FC80000, 0x71480000, 0x7149F2CA, 0x7149F2CA] and _bits(t[64]) == 0x7149F2CA      # the clamp
    t = dry_oracle.table(0.5, 1.0, 64)
    assert all(_bits(v) == 0 for v in t[:64]) and _bits(t[64]) == 0x3F000000


# ------------------------------------------------------------------------------------------ generate()'s gate
class DryDevice(ScriptedDevice):
    """the scripted device + a record of every sampling call: ("plain", slot) and ("dry", slot, m, b, a, start, breakers)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def set_sampling(self, *a, slot=None, **kw):
        self.calls.append(("plain", slot))
        super().set_sampling(*a, slot=slot, **kw)

    def set_dry(self, multiplier=0.0, base=1.75, allowed_length=2, start=0, breakers=(), slot=None):
        self.calls.append(("dry", slot, round(float(multiplier), 6), round(float(base), 6), int(allowed_length), int(start), tuple(breakers)))


def test_generate_takes_dry_and_refuses_bad_values():
    dev, proc = DryDevice(), fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0)
    T = int(ids.numel())
    kw = dict(input_ids=ids[None], pixel_values=px, bad_words_ids=[[IMG]], max_new_tokens=4, do_sample=True, seed=5)
    plain = dev.generate(**kw)
    assert dev.calls == [("plain", None)]
    dev.calls.clear()
    assert torch.equal(dev.generate(dry_multiplier=0.8, **kw), plain)      # (the toy LM ignores the sampler's parameters)
    assert dev.calls == [("plain", None), ("dry", None, 0.8, 1.75, 2, T, ())]          # the defaults; dry_start: the prompt length
    dev.calls.clear()
    dev.generate(dry_multiplier=2, dry_base=2.5, dry_allowed_length=4, dry_start=3, dry_sequence_breakers=[7, 9], do_sample=False,
                 **{k: v for k, v in kw.items() if k != "do_sample"})
    assert dev.calls == [("plain", None), ("dry", None, 2.0, 2.5, 4, 3, (7, 9))]       # greedy takes it as well
    dev.calls.clear()
    dev.generate(dry_multiplier=0.0, dry_base=3.0, **kw)        # off: no call
    dev.generate(dry_multiplier=None, dry_start=7, **kw)
    assert dev.calls == [("plain", None)] * 2
    dev.generation_config.dry_multiplier = 0.5                  # a checkpoint's generation_config.json is honoured
    dev.generation_config.dry_allowed_length = 3
    dev.calls.clear()
    dev.generate(**kw)
    assert dev.calls == [("plain", None), ("dry", None, 0.5, 1.75, 3, T, ())]
    del dev.generation_config.dry_multiplier, dev.generation_config.dry_allowed_length
    dev.calls.clear()
    for name, bads in (("dry_multiplier", (-0.1, 100.5, float("nan"), float("inf"), "1", True)),
                       ("dry_base", (0.99, 8.5, float("nan"), float("inf"), "2")),
                       ("dry_allowed_length", (0, 65, 2.0, "2", True)),
                       ("dry_start", (-1, 1.5)),
                       ("dry_sequence_breakers", ([-1], [VOCAB], list(range(17)), [1.5], "ab"))):
        for bad in bads:
            with pytest.raises(ValueError, match=name):
                dev.generate(**{"dry_multiplier": 0.8, name: bad}, **kw)
    assert dev.calls == []                                      # ... before anything runs
    assert check_dry() == (0.0, 1.75, 2, None, ())
    assert check_dry(100, 8, 64, 0, range(16)) == (100.0, 8.0, 64, 0, tuple(range(16)))
    # what stays refused stays refused
    with pytest.raises(NotImplementedError):
        dev.generate(repetition_penalty=1.2, dry_multiplier=0.8, **kw)
    with pytest.raises(NotImplementedError):
        dev.generate(no_repeat_ngram_size=3, **kw)
    # the plain scripted device (no such call on its "library") still decodes, and says so when asked for a value
    old = ScriptedDevice()
    assert torch.equal(old.generate(**kw), plain)
    with pytest.raises(_lib.DtkError, match="DRY"):
        old.generate(dry_multiplier=0.1, **kw)


def test_generator_starts_at_the_end_of_its_prompt():
    """DetikzifyGenerator(dry_multiplier=...): a rollout that continues a node carries dry_start = the length of the image prompt"""
    from detikzify_amd.infer import DetikzifyGenerator
    from .helpers import sketch_image
    dev, proc = DryDevice(), fake_processor(VOCAB, NIMG)
    gen = DetikzifyGenerator(dev, proc, sketch_image(0, 32), dry_multiplier=0.8, dry_allowed_length=3, max_length=60, do_sample=True,
                             temperature=1.0, top_p=1.0, top_k=0, metric=None)
    root = gen.montecarlo.root_node.token_ids
    node = torch.cat([root, torch.tensor([7, 8, 9], dtype=torch.int64)])
    gen.generate(node)
    assert dev.calls == [("plain", None), ("dry", None, 0.8, 1.75, 3, int(root.numel()), ())]
    dev.calls.clear()
    gen.generate(root, dry_start=0)
    assert dev.calls == [("plain", None), ("dry", None, 0.8, 1.75, 3, 0, ())]


# ------------------------------------------------------------------------------------------ the C ABI
NEW = {
    "dtk_set_dry": "(dtk_ctx* ctx, const dtk_dry* d)",
    "dtk_set_dry_slot": "(dtk_ctx* ctx, int slot, const dtk_dry* d)",
    "dtk_dry_history": "(dtk_ctx* ctx, int slot, int32_t* ids_out, int n_max)",
    "dtk_op_dry_scan": "(dtk_ctx* ctx, int V, const int64_t* history, int n_history, const int64_t* history2 /* or NULL */, int n_history2, "
                       "const dtk_dry* d, int32_t* ids_out, uint8_t* m_out, int n_max)",
    "dtk_op_sample_dry": "(dtk_ctx* ctx, const float* logits, int V, int step, int64_t* token_out, float* filtered_probs_out, "
                         "float* lp_out /* [2] or NULL */, const dtk_sampling_ext* x /* or NULL */, float presence, float frequency, "
                         "const int64_t* counted_ids, int n_counted, const int64_t* history, int n_history, const dtk_dry* d)",
    "dtk_engine_submit_dry": "(dtk_engine* e, dtk_join* j, const dtk_sampling_ext* x /* or NULL */, float presence, float frequency, int start, "
                             "const dtk_dry* d /* or NULL */, const int64_t* text_ids, int n_text, uint64_t text_key, uint64_t* ticket_out)",
    "dtk_engine_set_dry_op": "(dtk_engine* e, int (*set_dry_slot)(void* dev, int slot, const dtk_dry* d))",
}


def test_abi_is_additive_and_bound():
    assert _lib.DTK_ABI_VERSION == 7 and re.search(r"#define DTK_ABI_VERSION 7\b", HEADER)
    assert re.search(r"#define DTK_DRY_MAX_MATCH 64\b", HEADER) and re.search(r"#define DTK_DRY_MAX_BREAKERS 16\b", HEADER)
    assert (_lib.DTK_DRY_MAX_MATCH, _lib.DTK_DRY_MAX_BREAKERS) == (64, 16) == (dry_oracle.MAX_MATCH, dry_oracle.MAX_BREAKERS)
    flat = re.sub(r"\s+", " ", HEADER)
    X, F, I64, U64 = C.POINTER(_lib.DtkSamplingExt), C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    P, I, FL, D = C.c_void_p, C.c_int, C.c_float, C.POINTER(_lib.DtkDry)
    bound = {       # the header's parameter lists above, as ctypes (pointers to anything else: void*)
        "dtk_set_dry": [P, D],
        "dtk_set_dry_slot": [P, I, D],
        "dtk_dry_history": [P, I, C.POINTER(C.c_int32), I],
        "dtk_op_dry_scan": [P, I, I64, I, I64, I, D, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), I],
        "dtk_op_sample_dry": [P, P, I, I, I64, P, F, X, FL, FL, I64, I, I64, I, D],
        "dtk_engine_submit_dry": [P, C.POINTER(_lib.DtkJoin), X, FL, FL, I, D, I64, I, C.c_uint64, U64],
        "dtk_engine_set_dry_op": [P, _lib.DtkEngineOps.DRY],
    }
    for name, params in NEW.items():
        assert f"int {name}{params};" in flat.replace("int  ", "int "), name
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and list(args) == bound[name], name
    assert "int64_t dtk_dry_state_bytes(const dtk_ctx* ctx);" in flat and _lib.SYMBOLS["dtk_dry_state_bytes"] == (C.c_int64, [P])
    # dtk_op_sample_dry is dtk_op_sample_pen's signature plus the history and the struct
    assert list(_lib.SYMBOLS["dtk_op_sample_dry"][1][:-3]) == list(_lib.SYMBOLS["dtk_op_sample_pen"][1])
    assert _lib.DtkEngineOps.DRY._argtypes_ == (C.c_void_p, C.c_int, D)
    # the struct as the header lays it out
    m = re.search(r"typedef struct dtk_dry \{(.*?)\} dtk_dry;", HEADER, re.S)
    fields = [re.sub(r"\[.*", "", f.split()[-1]) for f in m.group(1).split(";") if f.strip()]
    assert fields == [n for n, _ in _lib.DtkDry._fields_]
    lib = _lib.load_library()
    assert lib.dtk_abi_version() == 7
    assert lib.dtk_abi_struct_size(14) == C.sizeof(_lib.DtkDry) == 84
    # the pinned layouts did not move
    assert lib.dtk_abi_struct_size(12) == C.sizeof(_lib.DtkSamplingExt) == 32
    assert lib.dtk_abi_struct_size(1) == C.sizeof(_lib.DtkSampling) == 136
    assert lib.dtk_abi_struct_size(6) == C.sizeof(_lib.DtkJoin)
    assert lib.dtk_abi_struct_size(15) == -1
    # null contexts / engines are an error code, not a crash
    d, tok, t = _lib.DtkDry(0.8, 1.75, 2, 0, 0), C.c_int64(), C.c_uint64()
    ids, ms, logits = (C.c_int32 * 4)(), (C.c_uint8 * 4)(), (C.c_float * 4)()
    assert lib.dtk_set_dry(None, C.byref(d)) == -1 and lib.dtk_set_dry_slot(None, 0, C.byref(d)) == -1
    assert lib.dtk_dry_history(None, -1, ids, 4) == -1
    assert lib.dtk_dry_state_bytes(None) == 0
    assert lib.dtk_op_dry_scan(None, 4, None, 0, None, 0, C.byref(d), ids, ms, 4) == -1
    assert lib.dtk_op_sample_dry(None, C.cast(logits, C.c_void_p), 4, 0, C.byref(tok), None, None, None, 0.0, 0.0, None, 0, None, 0,
                                 C.byref(d)) == -1
    assert lib.dtk_engine_submit_dry(None, C.byref(_lib.DtkJoin()), None, 0.0, 0.0, 0, C.byref(d), None, 0, 0, C.byref(t)) == -1
    assert lib.dtk_engine_set_dry_op(None, _lib.DtkEngineOps.DRY()) == -1


# ------------------------------------------------------------------------------------------ both engines
@pytest.mark.parametrize("engine", [NativeBatchEngine, BatchEngine], ids=["native", "python"])
def test_engines_carry_the_values_with_the_join_and_reset_them(engine):
    proc = fake_processor(VOCAB, NIMG)
    dev = DryDevice(slots=5)
    eng = engine(dev, max_batch=1, share_prefix=False)           # one decoding slot: every sequence takes slot 0
    try:
        ids, px = _prompt(proc, 1)
        T = int(ids.numel())
        kw = dict(input_ids=ids[None], pixel_values=px, bad_words_ids=[[IMG]], max_new_tokens=5, do_sample=True, eos_token_id=-1)
        a = dev.generate(seed=1, dry_multiplier=0.8, **kw)
        b = dev.generate(seed=2, **kw)
        c = dev.generate(seed=3, dry_multiplier=3.0, dry_base=2.0, dry_allowed_length=5, dry_start=2, dry_sequence_breakers=[4, 6], **kw)
    finally:
        eng.close()
    assert a.shape[1] == b.shape[1] == c.shape[1] == T + 5
    assert dev.calls == [("plain", 0), ("dry", 0, 0.8, 1.75, 2, T, ()), ("plain", 0), ("dry", 0, 0.0, 1.75, 2, 0, ()),
                         ("plain", 0), ("dry", 0, 3.0, 2.0, 5, 2, (4, 6))]
    # out of range never reaches the device
    dev2 = DryDevice(slots=5)
    eng = engine(dev2, max_batch=1, share_prefix=False)
    try:
        with pytest.raises(ValueError, match="dry_base"):
            with eng.sequence(ids, px, dict(do_sample=True, dry_multiplier=0.5, dry_base=0.5)):
                pass
        assert dev2.calls == []
    finally:
        eng.close()


def test_native_engine_without_the_op_refuses_a_join_with_values():
    """an engine of dtk_engine_create_ops that has no DRY op: a join with a multiplier fails in submit, one without joins"""
    proc = fake_processor(VOCAB, NIMG)
    dev = ScriptedDevice(slots=5)
    eng = NativeBatchEngine(dev, max_batch=2, share_prefix=False)
    lib = _lib.load_library()
    try:
        assert lib.dtk_engine_set_dry_op(eng._h, _lib.DtkEngineOps.DRY()) == 0       # take the op away again
        ids, px = _prompt(proc, 2)
        with pytest.raises(_lib.DtkError, match="dtk_engine_set_dry_op"):
            with eng.sequence(ids, px, dict(do_sample=True, seed=3, dry_multiplier=0.8), max_new_tokens=3):
                pass
        out = dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=3, do_sample=True, seed=3, eos_token_id=-1)
        assert out.shape[1] == ids.numel() + 3
        j, t = _lib.DtkJoin(), C.c_uint64()
        for bad in (_lib.DtkDry(101.0, 1.75, 2, 0, 0), _lib.DtkDry(float("nan"), 1.75, 2, 0, 0), _lib.DtkDry(0.8, 0.5, 2, 0, 0),
                    _lib.DtkDry(0.8, 1.75, 0, 0, 0), _lib.DtkDry(0.8, 1.75, 2, -1, 0), _lib.DtkDry(0.8, 1.75, 2, 0, 17)):
            assert lib.dtk_engine_submit_dry(eng._h, C.byref(j), None, 0.0, 0.0, 0, C.byref(bad), None, 0, 0, C.byref(t)) == -1
            assert b"dry_multiplier" in j.error_out
    finally:
        eng.close()
