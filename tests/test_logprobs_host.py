"""Log-probabilities of sampled tokens, host side (no GPU): the additive C ABI (include/dtk.h "Log-probabilities of sampled tokens"),
the shipped native run loop carrying a (logprob, sample_logprob) pair next to every token (dtk_engine_set_wait_lp_op /
dtk_engine_read_lp over a scripted device), and the Python layers above it — model.generate(return_logprobs=True) alone and inside
both batch engines — over the scripted device of tests/test_generate_loop.py.
"""
import ctypes as C
import math
import re
import threading
from pathlib import Path

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from detikzify_amd.infer.batching import BatchEngine
from detikzify_amd.infer.engine import NativeBatchEngine
from detikzify_amd.model.modeling import GenerateOutput

from .helpers import fake_processor
from .test_generate_loop import EOS, IMG, NIMG, VOCAB, ScriptedDevice, _prompt

NEW = ("dtk_decode_wait_lp", "dtk_decode_batch_wait_lp", "dtk_engine_read_lp", "dtk_engine_set_wait_lp_op", "dtk_op_sample_lp")
f32 = lambda v: float(np.float32(v))


# ------------------------------------------------------------------------------------------------ the ABI
def test_abi_is_additive():
    header = (Path(__file__).resolve().parents[1] / "include" / "dtk.h").read_text()
    lib = _lib.load_library()
    for name in NEW:
        assert re.search(r"^int\s+%s\(" % name, header, re.M), f"{name} is not declared in dtk.h"
        assert name in _lib.SYMBOLS and getattr(lib, name).argtypes is not None
    assert re.search(r"#define DTK_ABI_VERSION 7\b", header) and lib.dtk_abi_version() == 7 == _lib.DTK_ABI_VERSION
    # dtk_sampling / dtk_stats as they were before the feature
    assert lib.dtk_abi_struct_size(1) == C.sizeof(_lib.DtkSampling) == 136
    assert lib.dtk_abi_struct_size(2) == C.sizeof(_lib.DtkStats) == 104


# ------------------------------------------------------------------------------------------------ the native loop, raw
NEWLINE, STOP = 7, 2


def pair_of(script: int, i: int):
    """the scripted (logprob, sample_logprob) of token i of script `script`: distinct for every (script, i)"""
    return f32(-(script + 1) - i / 1024.0), f32(-(script + 1) * 16 - i / 512.0)


class RawDevice:
    """dtk_engine_ops in ctypes: a slot prefilled with ids[0] = k emits SCRIPTS[k] token by token, with pair_of(k, i)"""

    def __init__(self, scripts, slots=4, hold_after=None):
        self.scripts, self.which, self.pos, self.n_ids = scripts, {}, {}, {}
        # hold_after = (slot, script): once that slot has emitted the whole script, the next step is held back until `gate` is set
        self.steps, self.hold_after, self.gate = [], hold_after, threading.Event()
        O = _lib.DtkEngineOps

        def launch(dev, active):
            self.steps.append([s for s in range(_lib.DTK_MAX_BATCH) if active[s]])
            return 0

        def collect(out, lp=None, slp=None):
            if self.hold_after is not None:
                slot, k = self.hold_after
                if self.which.get(slot) == k and self.pos[slot] >= len(self.scripts[k]):
                    assert self.gate.wait(timeout=30)
            for s in range(_lib.DTK_MAX_BATCH):
                out[s] = -1
            for s in self.steps.pop(0):
                k, i = self.which[s], self.pos[s]
                out[s] = self.scripts[k][i] if i < len(self.scripts[k]) else 0     # (the step in flight behind a sequence's last one)
                if lp is not None:
                    lp[s], slp[s] = pair_of(k, i)
                self.pos[s] = i + 1
            return 0

        def prefill(dev, slot, ids, T, px, key, flags):
            self.which[slot], self.pos[slot], self.n_ids[slot] = int(ids[0]), 0, T
            return 0

        self.keep = [O.LAUNCH(launch), O.WAIT(lambda dev, out: collect(out)), O.PREFILL(prefill), O.SAMPLING(lambda dev, s, sp: 0),
                     O.FORK(lambda dev, a, b, n: 0), O.LCP(lambda dev, s, ids, n, key, out: 0), O.RESUME(lambda dev, s, ids, n, key: 0),
                     O.CTXLEN(lambda dev, s: self.n_ids.get(s, 0) + self.pos.get(s, 0)), O.LASTERR(lambda dev: None)]
        self.wait_lp = O.WAIT_LP(lambda dev, out, lp, slp: collect(out, lp, slp))
        self.ops = O(None, *self.keep, 4096, slots)


def _join(script: int, slot: int, budget: int):
    j = _lib.DtkJoin()
    ids = (C.c_int64 * 2)(script, 99)
    j.slot, j.n_ids, j.ids = slot, 2, C.cast(ids, C.c_void_p)
    j.prefix_src, j.max_new_tokens, j.n_stop, j.flush_mode, j.flush_max = -1, budget, 1, 1, 32
    j.stop_ids[0] = STOP
    j.sampling.temperature = j.sampling.top_p = 1.0
    return j, ids


def _read_all(lib, h, slot, cap, with_lp=True):
    toks, lps, slps, bursts = [], [], [], []
    buf, lp, slp = (C.c_int64 * cap)(), (C.c_float * cap)(), (C.c_float * cap)()
    n, state = C.c_int32(0), C.c_int32(0)
    while True:
        if with_lp:
            rc = lib.dtk_engine_read_lp(h, slot, buf, lp, slp, cap, C.byref(n), C.byref(state), 20000)
        else:
            rc = lib.dtk_engine_read(h, slot, buf, cap, C.byref(n), C.byref(state), 20000)
        assert rc == 0, rc
        toks += buf[:n.value]; lps += lp[:n.value]; slps += slp[:n.value]
        bursts.append(n.value)
        if state.value != _lib.DTK_SEQ_RUNNING:
            return toks, lps, slps, bursts
        assert n.value > 0, "dtk_engine_read_lp timed out"


def _scripts():
    plain = lambda n, base: [10 + (base + i) % 50 for i in range(n)]
    return [
        plain(40, 0) + [NEWLINE] + plain(9, 3) + [NEWLINE] + plain(100, 5),     # 0: a flush_max flush first, newline flushes, ends at its budget
        [NEWLINE] + plain(5, 1) + [NEWLINE] + plain(70, 2) + [STOP],            # 1: newline flushes, a flush_max flush, ends at its stop id
        plain(6, 9) + [NEWLINE] + plain(3, 4) + [STOP],                         # 2: short: ends while the others decode
        plain(33, 7) + [NEWLINE, STOP],                                         # 3: joins the slot sequence 2 left
    ]


def test_native_loop_delivers_every_pair_with_its_token():
    lib, scripts = _lib.load_library(), _scripts()
    dev = RawDevice(scripts, hold_after=(2, 2))
    h = C.c_void_p()
    assert lib.dtk_engine_create_ops(C.byref(dev.ops), C.byref(h)) == 0
    try:
        assert lib.dtk_engine_set_wait_lp_op(h, dev.wait_lp) == 0
        assert lib.dtk_engine_set_flush_tokens(h, (C.c_int64 * 1)(NEWLINE), 1) == 0
        budgets = {0: 140, 1: 500, 2: 500, 3: 500}
        keep = []
        assert lib.dtk_engine_expect(h, 3, 30000) == 0         # no step before the three have joined
        for k in range(3):
            j, ids = _join(k, k, budgets[k]); keep.append((j, ids))
            assert lib.dtk_engine_join(h, C.byref(j)) == 0, j.error_out
        # sequence 2 ends (its 11th step) while 0 and 1 decode; the device holds the next step back until sequence 3 has been queued
        t2, lp2, slp2, _ = _read_all(lib, h, 2, cap=4)
        assert lib.dtk_engine_leave(h, 2) == 0
        j3, ids3 = _join(3, 2, budgets[3])
        ticket = C.c_uint64(0)
        assert lib.dtk_engine_submit(h, C.byref(j3), C.byref(ticket)) == 0
        dev.gate.set()
        assert lib.dtk_engine_await(h, ticket.value) == 0, j3.error_out
        assert dev.which[0] == 0 and dev.pos[0] < 140, "sequence 0 was to be decoding still when sequence 3 joined"
        got = {2: (t2, lp2, slp2), 3: _read_all(lib, h, 2, cap=256)[:3], 0: _read_all(lib, h, 0, cap=7)[:3]}
        t1, _, _, _ = _read_all(lib, h, 1, cap=256, with_lp=False)        # the plain read on the same engine: the tokens, pairs dropped
        assert t1 == scripts[1]
        for k, (toks, lps, slps) in got.items():
            want = scripts[k][:budgets[k]]
            assert toks == want, k
            assert len(lps) == len(slps) == len(toks)
            for i in range(len(toks)):
                assert (lps[i], slps[i]) == pair_of(k, i), (k, i)
    finally:
        dev.gate.set()
        lib.dtk_engine_destroy(h)


def test_flushes_hand_out_pairs_in_step_with_tokens():
    """one sequence, read burst by burst: the first burst is the flush_max = 32 flush, later ones end at newlines, the last at the end"""
    lib, scripts = _lib.load_library(), _scripts()
    dev = RawDevice(scripts)
    h = C.c_void_p()
    assert lib.dtk_engine_create_ops(C.byref(dev.ops), C.byref(h)) == 0
    try:
        assert lib.dtk_engine_set_wait_lp_op(h, dev.wait_lp) == 0
        assert lib.dtk_engine_set_flush_tokens(h, (C.c_int64 * 1)(NEWLINE), 1) == 0
        j, ids = _join(0, 0, 140)
        assert lib.dtk_engine_join(h, C.byref(j)) == 0
        toks, lps, slps, bursts = _read_all(lib, h, 0, cap=256)
        assert toks == scripts[0][:140] and [(a, b) for a, b in zip(lps, slps)] == [pair_of(0, i) for i in range(140)]
        ends = np.cumsum(bursts)
        flush_points = {32, 41, 51, 83, 115, 140}       # flush_max, newline, newline, flush_max, flush_max, the budget
        assert ends[0] >= 32 and set(int(e) for e in ends if e) <= flush_points, bursts
    finally:
        lib.dtk_engine_destroy(h)


def test_engine_without_the_op_delivers_nan_pairs():
    lib, scripts = _lib.load_library(), _scripts()
    dev = RawDevice(scripts)
    h = C.c_void_p()
    assert lib.dtk_engine_create_ops(C.byref(dev.ops), C.byref(h)) == 0
    try:
        j, ids = _join(2, 1, 500)
        assert lib.dtk_engine_join(h, C.byref(j)) == 0
        toks, lps, slps, _ = _read_all(lib, h, 1, cap=5)
        assert toks == scripts[2] and len(lps) == len(toks)
        assert all(math.isnan(v) for v in lps) and all(math.isnan(v) for v in slps)
        n, state = C.c_int32(0), C.c_int32(0)
        buf, lp = (C.c_int64 * 4)(), (C.c_float * 4)()
        assert lib.dtk_engine_read_lp(h, 1, buf, lp, None, 4, C.byref(n), C.byref(state), 0) == -1      # one array without the other
    finally:
        lib.dtk_engine_destroy(h)


# ------------------------------------------------------------------------------------------------ generate() and the two engines
def lp_of(tok: int):
    return f32(-(tok % 97) / 8.0 - 0.125), f32(-(tok % 89) / 16.0)


class LpDevice(ScriptedDevice):
    """the scripted device with the log-probability wrappers of modeling.py scripted too: a token's pair is a function of the token"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.options = []

    def set_option(self, name, value):
        assert not self.bpending, "an option changed while a batched step is un-collected"
        self.options.append((name, value))

    def decode_wait_lp(self):
        assert ("logprobs", 1) in self.options
        tok = self.decode_wait()
        return (tok, *lp_of(tok))

    def decode_batch_wait_lp(self):
        assert ("logprobs", 1) in self.options
        toks = self.decode_batch_wait()
        pairs = [lp_of(t) if t >= 0 else (math.nan, math.nan) for t in toks]
        return toks, [p[0] for p in pairs], [p[1] for p in pairs]


KW = dict(bad_words_ids=[[IMG]], begin_suppress_tokens=[EOS], do_sample=True, max_length=NIMG + 60)


def _check_output(out, ids, plain):
    assert isinstance(out, GenerateOutput) and torch.equal(out.sequences, plain)
    new = out.sequences[0, ids.numel():].tolist()
    assert out.logprobs.shape == out.sample_logprobs.shape == (1, len(new))
    assert out.logprobs.dtype == out.sample_logprobs.dtype == torch.float32 and out.logprobs.device.type == "cpu"
    assert out.logprobs[0].tolist() == [lp_of(t)[0] for t in new]
    assert out.sample_logprobs[0].tolist() == [lp_of(t)[1] for t in new]


def test_generate_returns_pairs_aligned_with_the_new_tokens():
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 3, extra=[41])
    dev = LpDevice()
    plain = dev.generate(input_ids=ids[None], pixel_values=px, seed=5, **KW)
    assert isinstance(plain, torch.Tensor) and dev.options == [] and not dev.logprobs_enabled
    out = dev.generate(input_ids=ids[None], pixel_values=px, seed=5, return_logprobs=True, **KW)
    assert dev.options == [("logprobs", 1)] and dev.logprobs_enabled
    assert plain.shape[1] > ids.numel()
    _check_output(out, ids, plain)
    again = dev.generate(input_ids=ids[None], pixel_values=px, seed=5, **KW)       # the option stays on; the plain call is the plain tensor
    assert isinstance(again, torch.Tensor) and torch.equal(again, plain) and dev.options == [("logprobs", 1)]
    for name in ("output_scores", "output_logits", "return_dict_in_generate"):
        with pytest.raises(NotImplementedError):
            dev.generate(input_ids=ids[None], pixel_values=px, seed=5, **{name: True}, **KW)
    # a prompt that leaves no room: no new token, empty pair tensors
    none = dev.generate(input_ids=ids[None], pixel_values=px, seed=5, return_logprobs=True, max_new_tokens=0, **{k: v for k, v in KW.items() if k != "max_length"})
    assert none.sequences.shape[1] == ids.numel() and none.logprobs.shape == (1, 0)


@pytest.mark.parametrize("make", [NativeBatchEngine, BatchEngine], ids=lambda m: m.__name__)
def test_both_engines_deliver_the_pairs_of_the_sequence_alone(make):
    proc = fake_processor(VOCAB, NIMG)
    jobs = []
    for j in range(12):
        ids, px = _prompt(proc, j % 3, extra=[40 + j, 50 + j][: j % 3])
        jobs.append((ids, px, 200 + j))
    alone_dev = LpDevice()
    alone = [alone_dev.generate(input_ids=i[None], pixel_values=p, seed=s, **KW) for i, p, s in jobs]
    dev = LpDevice(slots=5)
    eng = make(dev, max_batch=4)
    got, errs = [None] * len(jobs), []

    def worker(k):
        try:
            for j in range(k, len(jobs), 6):
                i, p, s = jobs[j]
                got[j] = dev.generate(input_ids=i[None], pixel_values=p, seed=s, return_logprobs=(j % 4 != 3), **KW)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    try:
        # the first sequence asks for log-probabilities while every slot is free: the device is switched over before the first join
        got[0] = dev.generate(input_ids=jobs[0][0][None], pixel_values=jobs[0][1], seed=jobs[0][2], return_logprobs=True, **KW)
        assert dev.options == [("logprobs", 1)]
        ths = [threading.Thread(target=worker, args=(k,)) for k in range(6)]
        [t.start() for t in ths]
        [t.join(timeout=90) for t in ths]
        assert not any(t.is_alive() for t in ths), "threads hang"
        assert not errs, errs[:1]
    finally:
        eng.close()
    assert dev.options == [("logprobs", 1)]
    for j, (a, g, (ids, _, _)) in enumerate(zip(alone, got, jobs)):
        if j % 4 == 3:
            assert isinstance(g, torch.Tensor) and torch.equal(a, g)       # a sequence without the flag in the same batch
        else:
            _check_output(g, ids, a)


def test_logprobs_are_not_switched_on_under_running_sequences():
    """a device whose option is off and whose slots are held refuses the switch in both engines (the C side would refuse it too)"""
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 1)
    for make in (NativeBatchEngine, BatchEngine):
        dev = LpDevice(slots=5)
        eng = make(dev, max_batch=4)
        try:
            with eng.sequence(ids, px, dict(do_sample=False), max_new_tokens=4):
                with pytest.raises(_lib.DtkError, match="before the first join"):
                    dev.generate(input_ids=ids[None], pixel_values=px, seed=1, return_logprobs=True, **KW)
            assert dev.options == []
        finally:
            eng.close()
