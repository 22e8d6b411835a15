"""Top-k alternatives in the batch engines, host side (no GPU): the additive C ABI, the native loop's per-token records
(dtk_engine_read_top) on a stub device, and both engines, generate() and simulate_parallel on the scripted device of
tests/test_generate_loop.py with the top-k wrappers of modeling.py scripted too."""
import ctypes as C
import math
import re
import threading
from pathlib import Path

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from detikzify_amd.infer import DetikzifyPipeline, SyntheticTikzDocument
from detikzify_amd.infer.batching import BatchEngine, make_engine, simulate_parallel
from detikzify_amd.infer.engine import NativeBatchEngine
from detikzify_amd.model.modeling import GenerateOutput

from .helpers import fake_processor, sketch_image
from .test_generate_loop import EOS, IMG, NIMG, VOCAB, ScriptedDevice, _prompt
from .test_logprobs_host import NEWLINE, STOP, RawDevice, _join, lp_of, pair_of

TOP = _lib.DTK_MAX_TOP
NEW = ("dtk_engine_read_top", "dtk_engine_set_wait_top_op", "dtk_op_top_logits")
f32 = lambda v: float(np.float32(v))


def test_abi_is_additive():
    header = (Path(__file__).resolve().parents[1] / "include" / "dtk.h").read_text()
    lib = _lib.load_library()
    for name in NEW:
        assert re.search(r"^int\s+%s\(" % name, header, re.M), f"{name} is not declared in dtk.h"
        assert name in _lib.SYMBOLS and getattr(lib, name).argtypes is not None
    assert re.search(r"^#define DTK_ABI_VERSION 7\b", header, re.M) and lib.dtk_abi_version() == 7 == _lib.DTK_ABI_VERSION
    assert lib.dtk_abi_struct_size(8) == C.sizeof(_lib.DtkEngineOps)       # the op came through a setter: the struct is what it was


# ------------------------------------------------------------------------------------------------ the native loop, raw
def rec_of(script: int, i: int, k: int = 3):
    """the scripted record of token i of script `script`: k entries, distinct for every (script, i, entry); (-1, NaN) beyond k"""
    ids = [1000 * script + 8 * i + e for e in range(k)] + [-1] * (TOP - k)
    lps = [f32(-(script + 1) - i / 256.0 - e / 4096.0) for e in range(k)] + [math.nan] * (TOP - k)
    return ids, lps


def same(a, b):
    return len(a) == len(b) and all((math.isnan(x) and math.isnan(y)) or x == y for x, y in zip(a, b))


class RawTopDevice(RawDevice):
    """RawDevice + the wait-top op: the step's tokens and pairs as there, rec_of(script, i) for every slot that took part"""

    def __init__(self, scripts, slots=4, hold_launch=None):
        super().__init__(scripts, slots=slots)
        wait_lp = self.wait_lp
        if hold_launch is not None:      # the hold_launch-th launch (from 0) waits until `gate` is set
            inner, self.launched = self.keep[0], 0

            def launch(dev, active):
                if self.launched == hold_launch:
                    assert self.gate.wait(timeout=30)
                self.launched += 1
                return inner(dev, active)
            self.keep[0] = _lib.DtkEngineOps.LAUNCH(launch)
            self.ops = _lib.DtkEngineOps(None, *self.keep, 4096, slots)

        def wait_top(dev, out, lp, slp, ti, tl):
            active = list(self.steps[0])
            at = {s: self.pos[s] for s in active}
            rc = wait_lp(dev, out, lp, slp)
            for s in range(_lib.DTK_MAX_BATCH):
                ids, lps = rec_of(self.which[s], at[s]) if s in at else ([-1] * TOP, [math.nan] * TOP)
                for e in range(TOP):
                    ti[s * TOP + e], tl[s * TOP + e] = ids[e], lps[e]
            return rc
        self.wait_top = _lib.DtkEngineOps.WAIT_TOP(wait_top)


def _read_top(lib, h, slot, cap):
    toks, lps, slps, tis, tls = [], [], [], [], []
    buf, lp, slp = (C.c_int64 * cap)(), (C.c_float * cap)(), (C.c_float * cap)()
    ti, tl = (C.c_int32 * (cap * TOP))(), (C.c_float * (cap * TOP))()
    n, state = C.c_int32(0), C.c_int32(0)
    while True:
        rc = lib.dtk_engine_read_top(h, slot, buf, lp, slp, ti, tl, cap, C.byref(n), C.byref(state), 20000)
        assert rc == 0, rc
        toks += buf[:n.value]; lps += lp[:n.value]; slps += slp[:n.value]
        for i in range(n.value):
            tis.append(list(ti[i * TOP:(i + 1) * TOP])); tls.append(list(tl[i * TOP:(i + 1) * TOP]))
        if state.value != _lib.DTK_SEQ_RUNNING:
            return toks, lps, slps, tis, tls
        assert n.value > 0, "dtk_engine_read_top timed out"


@pytest.mark.parametrize("length", [1, 3, 32])
def test_records_travel_token_by_token(length):
    """three sequences of `length` tokens in one engine, each read with another buffer size: record i is token i's"""
    lib = _lib.load_library()
    scripts = [[10 + (7 * k + i) % 50 for i in range(length - 1)] + [STOP] for k in range(3)]
    dev = RawTopDevice(scripts)
    h = C.c_void_p()
    assert lib.dtk_engine_create_ops(C.byref(dev.ops), C.byref(h)) == 0
    try:
        assert lib.dtk_engine_set_wait_top_op(h, dev.wait_top) == 0
        assert lib.dtk_engine_set_flush_tokens(h, (C.c_int64 * 1)(NEWLINE), 1) == 0
        keep = []
        assert lib.dtk_engine_expect(h, 3, 30000) == 0
        for k in range(3):
            j, ids = _join(k, k, 500); keep.append((j, ids))
            assert lib.dtk_engine_join(h, C.byref(j)) == 0, j.error_out
        for k, cap in ((0, 256), (1, 1), (2, 5)):
            toks, lps, slps, tis, tls = _read_top(lib, h, k, cap)
            assert toks == scripts[k] and len(tis) == len(tls) == len(toks) == length
            for i in range(length):
                assert (lps[i], slps[i]) == pair_of(k, i)
                assert tis[i] == rec_of(k, i)[0] and same(tls[i], rec_of(k, i)[1]), (k, i)
    finally:
        lib.dtk_engine_destroy(h)


def test_an_engine_that_collects_none_refuses_the_call():
    lib = _lib.load_library()
    scripts = [[10 + i for i in range(6)] + [NEWLINE] + [20 + i for i in range(5)] + [STOP]]
    dev = RawTopDevice(scripts)
    h = C.c_void_p()
    assert lib.dtk_engine_create_ops(C.byref(dev.ops), C.byref(h)) == 0
    try:
        n, state = C.c_int32(0), C.c_int32(0)
        buf, lp, slp = (C.c_int64 * 64)(), (C.c_float * 64)(), (C.c_float * 64)()
        ti, tl = (C.c_int32 * (64 * TOP))(), (C.c_float * (64 * TOP))()
        j, ids = _join(0, 0, 500)
        assert lib.dtk_engine_join(h, C.byref(j)) == 0, j.error_out
        assert lib.dtk_engine_read_top(h, 0, buf, lp, slp, ti, tl, 64, C.byref(n), C.byref(state), 0) == -1      # DTK_ERR_ARG
        assert lib.dtk_engine_set_wait_top_op(h, dev.wait_top) == 0
        # one array without the other, and records without the pairs
        assert lib.dtk_engine_read_top(h, 0, buf, lp, slp, ti, None, 64, C.byref(n), C.byref(state), 0) == -1
        assert lib.dtk_engine_read_top(h, 0, buf, None, None, ti, tl, 64, C.byref(n), C.byref(state), 0) == -1
        toks = _read_top(lib, h, 0, 64)[0]
        assert toks == scripts[0]
    finally:
        lib.dtk_engine_destroy(h)


def test_an_op_given_mid_sequence_leaves_the_earlier_tokens_without_records():
    lib = _lib.load_library()
    scripts = [[10 + i % 40 for i in range(40)] + [STOP]]
    dev = RawTopDevice(scripts, hold_launch=4)       # (two steps are in flight: the first tokens are collected without the op)
    h = C.c_void_p()
    assert lib.dtk_engine_create_ops(C.byref(dev.ops), C.byref(h)) == 0
    try:
        n, state = C.c_int32(0), C.c_int32(0)
        buf = (C.c_int64 * 256)()
        j, ids = _join(0, 0, 500)
        j.flush_mode = 0                         # every token wakes the reader
        assert lib.dtk_engine_join(h, C.byref(j)) == 0, j.error_out
        assert lib.dtk_engine_read(h, 0, buf, 3, C.byref(n), C.byref(state), 20000) == 0 and n.value >= 1
        first = list(buf[:n.value])
        assert lib.dtk_engine_set_wait_top_op(h, dev.wait_top) == 0
        dev.gate.set()
        toks, lps, slps, tis, tls = _read_top(lib, h, 0, 256)
        toks = first + toks
        assert toks == scripts[0]
        off = len(first)
        began = next(i for i, r in enumerate(tis) if r[0] != -1)
        assert off + began <= 4, "the steps launched behind the gate are collected through the op"
        for i, (ri, rl) in enumerate(zip(tis, tls)):
            if i < began:       # produced before the op was there: (-1, NaN) throughout, pairs NaN
                assert ri == [-1] * TOP and all(math.isnan(v) for v in rl) and math.isnan(lps[i])
            else:
                assert ri == rec_of(0, off + i)[0] and same(rl, rec_of(0, off + i)[1]) and lps[i] == pair_of(0, off + i)[0]
    finally:
        dev.gate.set()
        lib.dtk_engine_destroy(h)


# ------------------------------------------------------------------------------------------------ generate() and the two engines
def top_of(tok: int, k: int):
    """the scripted record of a step that sampled `tok`: k ids and k log-probabilities, functions of the token"""
    return [(tok + 3 * e) % VOCAB for e in range(k)], [f32(-(tok % 97) / 8.0 - 0.125 - e / 64.0) for e in range(k)]


class TopDevice(ScriptedDevice):
    """the scripted device with the log-probability and top-k wrappers of modeling.py scripted too"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.options = []

    def set_option(self, name, value):
        assert not self.bpending, "an option changed while a batched step is un-collected"
        self.options.append((name, value))

    def synchronize(self):
        pass

    def _k(self):
        k = next((v for n, v in reversed(self.options) if n == "top_logprobs"), 0)
        assert k > 0 and dict(self.options).get("logprobs") == 1, "a top-k wait on a device that was not switched over"
        return k

    def decode_wait(self, top=False):
        tok = super().decode_wait()
        return (tok, *lp_of(tok), *top_of(tok, self._k())) if top else tok

    def decode_batch_wait_lp(self):
        toks = super().decode_batch_wait()
        pairs = [lp_of(t) if t >= 0 else (math.nan, math.nan) for t in toks]
        return toks, [p[0] for p in pairs], [p[1] for p in pairs]

    def decode_batch_wait(self, top=False):
        if not top:
            return super().decode_batch_wait()
        k = self._k()
        toks, lps, slps = self.decode_batch_wait_lp()
        recs = [top_of(t, k) if t >= 0 else ([-1] * k, [math.nan] * k) for t in toks]
        return toks, lps, slps, [r[0] for r in recs], [r[1] for r in recs]


KW = dict(bad_words_ids=[[IMG]], begin_suppress_tokens=[EOS], do_sample=True, max_length=NIMG + 60)
ENGINES = pytest.mark.parametrize("make", [NativeBatchEngine, BatchEngine], ids=lambda m: m.__name__)


def _check(out, ids, plain, j):
    assert isinstance(out, GenerateOutput) and torch.equal(out.sequences, plain)
    new = out.sequences[0, ids.numel():].tolist()
    assert out.top_ids.shape == out.top_logprobs.shape == (1, len(new), j)
    assert out.top_ids.dtype == torch.int64 and out.top_logprobs.dtype == torch.float32
    assert out.logprobs[0].tolist() == [lp_of(t)[0] for t in new]
    assert out.top_ids[0].tolist() == [top_of(t, j)[0] for t in new]
    assert out.top_logprobs[0].tolist() == [top_of(t, j)[1] for t in new]


@ENGINES
def test_both_engines_deliver_the_records_of_the_sequence_alone(make):
    proc = fake_processor(VOCAB, NIMG)
    jobs = []
    for n in range(12):
        ids, px = _prompt(proc, n % 3, extra=[40 + n, 50 + n][: n % 3])
        jobs.append((ids, px, 300 + n))
    alone_dev = TopDevice()
    alone = [alone_dev.generate(input_ids=i[None], pixel_values=p, seed=s, **KW) for i, p, s in jobs]
    dev = TopDevice(slots=5)
    eng = make(dev, max_batch=4, top_logprobs=3)
    assert dev.options == [("logprobs", 1), ("top_logprobs", 3)] and dev.top_logprobs_enabled == 3
    got, errs = [None] * len(jobs), []
    want_j = lambda n: (3, 2, 1, 0)[n % 4]      # the engine's k, fewer columns, one column, a sequence that asks for none

    def worker(k):
        try:
            for n in range(k, len(jobs), 6):
                i, p, s = jobs[n]
                j = want_j(n)
                got[n] = dev.generate(input_ids=i[None], pixel_values=p, seed=s, return_logprobs=bool(j), **({"top_logprobs": j} if j else {}), **KW)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    try:
        ths = [threading.Thread(target=worker, args=(k,)) for k in range(6)]
        [t.start() for t in ths]
        [t.join(timeout=90) for t in ths]
        assert not any(t.is_alive() for t in ths), "threads hang"
        assert not errs, errs[:1]
        # j > k: a ValueError that names the engine's k, before a slot is taken
        with pytest.raises(ValueError, match="top_logprobs=3"):
            dev.generate(input_ids=jobs[0][0][None], pixel_values=jobs[0][1], seed=1, return_logprobs=True, top_logprobs=4, **KW)
        with pytest.raises(ValueError, match="return_logprobs"):
            with eng.sequence(jobs[0][0], jobs[0][1], dict(do_sample=False), max_new_tokens=4, top_logprobs=2):
                pass
        assert not eng.busy()
    finally:
        eng.close()
    # close() restores what the constructor found: both options off again
    assert dev.options == [("logprobs", 1), ("top_logprobs", 3), ("top_logprobs", 0), ("logprobs", 0)]
    assert dev.top_logprobs_enabled == 0 and not dev.logprobs_enabled and dev.batch_engine is None
    for n, (a, g, (ids, _, _)) in enumerate(zip(alone, got, jobs)):
        if want_j(n) == 0:
            assert isinstance(g, torch.Tensor) and torch.equal(a, g)
        else:
            _check(g, ids, a, want_j(n))


@ENGINES
def test_close_restores_options_that_were_on_and_an_engine_without_the_argument_still_refuses(make):
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 1)
    dev = TopDevice(slots=5)
    dev.enable_top_logprobs(2)
    eng = make(dev, max_batch=4, top_logprobs=5)
    try:
        assert dev.top_logprobs_enabled == 5
        out = dev.generate(input_ids=ids[None], pixel_values=px, seed=4, return_logprobs=True, top_logprobs=5, **KW)
        assert out.top_ids.shape[2] == 5
    finally:
        eng.close()
    assert dev.top_logprobs_enabled == 2 and dev.logprobs_enabled
    assert dev.options == [("logprobs", 1), ("top_logprobs", 2), ("top_logprobs", 5), ("top_logprobs", 2)]
    for bad in (0, 9):
        with pytest.raises(ValueError, match="top_logprobs"):
            make(dev, max_batch=4, top_logprobs=bad)
    assert dev.batch_engine is None
    plain = make(dev, max_batch=4)
    try:
        with pytest.raises(NotImplementedError, match="top_logprobs: not in the batch engines yet"):
            with plain.sequence(ids, px, dict(do_sample=False), max_new_tokens=4, logprobs=True, top_logprobs=2):
                pass
    finally:
        plain.close()
    assert dev.top_logprobs_enabled == 2 and dev.logprobs_enabled


def test_make_engine_takes_the_argument():
    dev = TopDevice(slots=5)
    eng = make_engine(dev, max_batch=4, top_logprobs=4)
    try:
        assert eng.top_logprobs == 4 and dev.top_logprobs_enabled == 4
    finally:
        eng.close()
    assert dev.top_logprobs_enabled == 0


def test_simulate_parallel_attaches_the_fields_to_every_document():
    proc = fake_processor(VOCAB, NIMG)
    dev = TopDevice(slots=5)
    pipe = DetikzifyPipeline(dev, proc, metric="fast", compile_timeout=None, document_class=SyntheticTikzDocument,
                             max_length=NIMG + 40)
    docs = list(simulate_parallel(pipe, sketch_image(2, 96), trees=3, expansions_per_tree=3, top_logprobs=2))
    assert len(docs) == 9
    assert dev.top_logprobs_enabled == 0 and not dev.logprobs_enabled and dev.batch_engine is None
    seen = 0
    for score, doc in docs:
        n = len(doc.token_top_ids)
        assert n == len(doc.token_top_logprobs) == len(doc.token_logprobs) == len(doc.token_sample_logprobs) and n > 0
        toks = [row[0] for row in doc.token_top_ids]       # (entry 0 of a scripted record is the sampled token itself)
        assert proc.decode(torch.tensor(toks), skip_special_tokens=True) == doc.code
        for t, row_i, row_l, lp, slp in zip(toks, doc.token_top_ids, doc.token_top_logprobs, doc.token_logprobs, doc.token_sample_logprobs):
            assert row_i == top_of(t, 2)[0] and row_l == top_of(t, 2)[1] and (lp, slp) == lp_of(t)
            seen += 1
    assert seen > 20
    # trees = 1 is the sequential search: the same fields, through the single-sequence steps
    score, doc = next(iter(pipe.simulate(sketch_image(2, 96), expansions=1, top_logprobs=2)))
    assert len(doc.token_top_ids) == len(doc.token_logprobs) > 0 and all(len(r) == 2 for r in doc.token_top_ids)
