"""Guided sequences in the native batch engine, on the CPU: the run loop is the shipped native code (csrc/dtk_engine.cpp), the device
under it the scripted PairDevice of tests/cfg_engine_cases.py, which keeps pairs the way the library does and refuses what the library
refuses (half a pair in a step, a pair in two phases, a pair table written with a step in flight).  What this pins without a GPU:

  * the ABI grew additively (version 7, the new symbols, dtk_abi_struct_size(18), the pinned -1 cases);
  * a guided join is both prompts in, then set_guidance, then steps that contain both slots or neither;
  * the pair resumes in place only if both slots hold their prompts; the forced token is dropped once, `resumed` counts once;
  * a stop id on the leader or leave(cond) ends both slots; a follower slot refuses read and leave;
  * a disagreement of the two tokens stops the engine with the pair named;
  * a failure in the second half of a join leaves no pair and both slots free; stale pairs are dissolved before a slot is re-used;
  * NativeBatchEngine and the Python-driven BatchEngine alike: guided_pairs=0 keeps the refusal, slot accounting with an odd number of free slots, one negative prefix encode
    for N guided sequences of N images, and guided generate() under the engine is guided generate() without one.
"""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from detikzify_amd import _lib
from detikzify_amd.infer.batching import BatchEngine
from detikzify_amd.infer.engine import NativeBatchEngine

from .cfg_engine_cases import EOS, IMG, NIMG, VOCAB, PairDevice, prompt, threads
from .helpers import fake_processor

NEW = ("dtk_reserve_guidance", "dtk_batch_graph_captures", "dtk_engine_submit_guided", "dtk_engine_set_guidance_op")
ERR_ARG, ERR_STATE = -1, -3          # include/dtk.h
KW = dict(bad_words_ids=[[IMG]], begin_suppress_tokens=[EOS], do_sample=True)


def test_abi_is_additive():
    lib = _lib.load_library()
    header = (Path(__file__).resolve().parents[1] / "include" / "dtk.h").read_text()
    assert lib.dtk_abi_version() == 7 == _lib.DTK_ABI_VERSION and re.search(r"#define DTK_ABI_VERSION 7\b", header)
    for name in NEW:
        assert name in _lib.SYMBOLS and re.search(rf"\b{name}\(", header), name
        assert getattr(lib, name).argtypes is not None
    assert lib.dtk_abi_struct_size(18) == C.sizeof(_lib.DtkGuided) == 40
    for which in (13, 15, 17, 99):
        assert lib.dtk_abi_struct_size(which) == -1, which
    assert lib.dtk_abi_struct_size(6) == C.sizeof(_lib.DtkJoin) and lib.dtk_abi_struct_size(7) == C.sizeof(_lib.DtkEngineStats)
    assert lib.dtk_abi_struct_size(2) == 104


ENGINES = pytest.mark.parametrize("make", [NativeBatchEngine, BatchEngine], ids=["native", "python"])


def _engine(make=NativeBatchEngine, slots=9, pairs=2, **kw):
    dev = PairDevice(slots=slots)
    return dev, make(dev, max_batch=kw.pop("max_batch", 4), guided_pairs=pairs, **kw)


def _guided(dev, ids, px, neg_px, seed, scale=2.0, owner=None, **kw):
    return dev.generate(input_ids=ids[None], pixel_values=px, seed=seed, guidance_scale=scale, negative_pixel_values=neg_px,
                        sequence_owner=owner, **{**KW, **kw})


def _alone(ids, px, neg_px, seed, scale=2.0, **kw):
    return _guided(PairDevice(slots=2), ids, px, neg_px, seed, scale, **kw)


@ENGINES
def test_call_order_of_a_guided_join_and_its_steps(make):
    proc = fake_processor(VOCAB, NIMG)
    ids, px = prompt(proc, 0, extra=[40, 41])
    white = torch.ones_like(px)
    ref = _alone(ids, px, white, 7, max_new_tokens=12)
    dev, eng = _engine(make)
    assert ("reserve_guidance", 2) in dev.log
    out = _guided(dev, ids, px, white, 7, max_new_tokens=12)
    st = eng.stats()
    eng.close()
    assert torch.equal(out, ref)
    names = [e[0] for e in dev.log]
    k = names.index("set_guidance")
    c, u, g = dev.log[k][1:]
    assert g == 2.0 and c != u
    # both prompts are in before the pair is set, and no step before it
    before = dev.log[:k]
    assert "launch" not in names[:k]
    filled = {e[1] for e in before if e[0] == "prefill"} | {e[2] for e in before if e[0] == "kv_fork"}
    assert {c, u} <= filled
    # the unconditional slot: neutral greedy sampling (the last set_sampling of that slot before the pair)
    assert [e for e in before if e[0] == "set_sampling" and e[1] == u][-1][2] is False
    assert [e for e in before if e[0] == "set_sampling" and e[1] == c][-1][2] is True
    steps = [e[1] for e in dev.log[k:] if e[0] == "launch"]
    assert steps and all((c in s) == (u in s) for s in steps) and all(c in s for s in steps)
    new = out.shape[1] - ids.numel()
    assert st["tokens_out"] == new and st["joins"] == 1          # one token per pair per step, one sequence
    assert sorted(eng.free) == [0, 1, 2, 3]
    # closing the engine dissolved the pair it left and gave the reservation back
    assert dev.pairs == {} and dev.log[-1] == ("reserve_guidance", 0)


@ENGINES
@pytest.mark.parametrize("both", [True, False])
def test_a_pair_resumes_only_if_both_slots_hold_their_prompt(make, both):
    proc = fake_processor(VOCAB, NIMG)
    ids, px = prompt(proc, 1, extra=[60])
    white = torch.ones_like(px)
    kw = dict(eos_token_id=-1, suppress_tokens=[EOS])
    first = _alone(ids, px, white, 11, max_new_tokens=12, **kw)
    ids2 = first[0, : ids.numel() + 6]
    ref_dev = PairDevice(slots=2)
    second = _guided(ref_dev, ids2, px, white, 12, max_new_tokens=8, **kw)
    dev, eng = _engine(make)
    assert torch.equal(_guided(dev, ids, px, white, 11, owner=5, max_new_tokens=12, **kw), first)
    u = next(e for e in dev.log if e[0] == "set_guidance")[2]
    if not both:            # something else went through the unconditional slot meanwhile: it no longer holds its prompt
        dev.ctx[u] = dev.ctx[u][:NIMG] + [99]
    n0 = len(dev.log)
    got = _guided(dev, ids2, px, white, 12, owner=5, max_new_tokens=8, **kw)
    st = eng.stats()
    nat = eng.native_stats() if make is NativeBatchEngine else dict(resumed=st["resumed_in_place"], tokens_out=st["tokens_out"])
    eng.close()
    log = dev.log[n0:]
    resumed = [e for e in log if e[0] == "resume"]
    if both:
        assert len(resumed) == 2 and not [e for e in log if e[0] == "prefill"]
        assert st["resumed_in_place"] == 1 and nat["resumed"] == 1
        assert torch.equal(got, second)      # the forced token was dropped once: the new tokens start behind the prompt
    else:
        assert not resumed and st["resumed_in_place"] == 0 and nat["resumed"] == 0
        assert len([e for e in log if e[0] == "prefill"]) == 2
        assert got.shape[1] == ids2.numel() + 8 and torch.equal(got[0, : ids2.numel()], ids2)
    assert nat["tokens_out"] == 12 + 8


def _raw_engine(dev, decode_slots=4):
    """the native loop over the scripted device, driven through the C entry points themselves"""
    eng = NativeBatchEngine(dev, max_batch=decode_slots, guided_pairs=decode_slots // 2, share_prefix=False)
    return eng, eng.lib, eng._h


def _join(ids, slot, px=None, n_new=8, stops=(), do_sample=True, seed=1, try_resume=0, key=0):
    j = _lib.DtkJoin()
    j.slot, j.n_ids, j.ids = slot, int(ids.numel()), ids.data_ptr()
    j.pixels, j.image_key, j.prefix_src, j.try_resume = None, key, -1, try_resume
    j.sampling.do_sample, j.sampling.temperature, j.sampling.top_p, j.sampling.seed = int(do_sample), 1.0, 1.0, seed
    j.max_new_tokens, j.n_stop = n_new, len(stops)
    for i, t in enumerate(stops):
        j.stop_ids[i] = t
    return j


def _submit_guided(lib, h, jc, ju, scale=2.0):
    g = _lib.DtkGuided()
    g.cond, g.uncond, g.scale = C.pointer(jc), C.pointer(ju), scale
    t = C.c_uint64(0)
    rc = lib.dtk_engine_submit_guided(h, C.byref(g), None, C.c_float(0), C.c_float(0), 0, None, None, None, None, 0, None, 0, C.c_uint64(0),
                                      C.byref(t))
    return rc if rc else lib.dtk_engine_await(h, t.value)


def _read_all(lib, h, slot):
    buf, n, state, out = (C.c_int64 * 64)(), C.c_int32(0), C.c_int32(0), []
    while True:
        rc = lib.dtk_engine_read(h, slot, buf, 64, C.byref(n), C.byref(state), 5000)
        if rc:
            return rc, out, state.value
        out += buf[: n.value]
        if state.value != _lib.DTK_SEQ_RUNNING:
            return 0, out, state.value


def test_stop_leave_and_the_follower_slot():
    dev = PairDevice(slots=5)
    eng, lib, h = _raw_engine(dev)
    a, b = torch.arange(10, 20), torch.arange(30, 38)
    # find the leader's third token, then make it the stop id
    jc, ju = _join(a, 0, n_new=6), _join(b, 1)
    assert _submit_guided(lib, h, jc, ju) == 0 and (jc.how_out, ju.how_out) == (_lib.DTK_JOIN_FULL, _lib.DTK_JOIN_FULL)
    rc, toks, state = _read_all(lib, h, 0)
    assert rc == 0 and len(toks) == 6 and state == _lib.DTK_SEQ_FINISHED
    buf, n, st_ = (C.c_int64 * 8)(), C.c_int32(0), C.c_int32(0)
    assert lib.dtk_engine_read(h, 1, buf, 8, C.byref(n), C.byref(st_), 0) == ERR_ARG       # a follower slot refuses read
    assert lib.dtk_engine_leave(h, 1) == ERR_ARG                                           # ... and leave
    assert lib.dtk_engine_leave(h, 0) == 0
    lib.dtk_engine_set_option(h, b"drain", 0)
    stop = toks[2]
    n0 = len(dev.log)
    jc, ju = _join(a, 0, n_new=6, stops=[stop]), _join(b, 1)
    assert _submit_guided(lib, h, jc, ju) == 0
    rc, toks2, state = _read_all(lib, h, 0)
    assert rc == 0 and toks2 == toks[:3] and state == _lib.DTK_SEQ_FINISHED      # the stop id ended the leader ...
    lib.dtk_engine_leave(h, 0)
    lib.dtk_engine_set_option(h, b"drain", 0)
    steps = [e[1] for e in dev.log[n0:] if e[0] == "launch"]
    assert len(steps) <= 3 + 2 and all(s == (0, 1) for s in steps)               # ... and its follower in the same collect
    assert len(dev.ctx[0]) - a.numel() == len(dev.ctx[1]) - b.numel() == len(steps)
    st = eng.native_stats()
    assert st["wasted_slot_steps"] == 2 * (len(steps) - 3)                       # the steps in flight count both slots
    # leave(cond) frees both: the two slots take a new pair, the other way round
    jc, ju = _join(a, 1, n_new=50), _join(b, 0)
    assert _submit_guided(lib, h, jc, ju) == 0
    assert lib.dtk_engine_leave(h, 1) == 0
    lib.dtk_engine_set_option(h, b"drain", 0)
    jc, ju = _join(a, 2, n_new=2), _join(b, 0)
    assert _submit_guided(lib, h, jc, ju) == 0, jc.error_out
    assert _read_all(lib, h, 2)[0] == 0
    lib.dtk_engine_leave(h, 2)
    eng.close()


def test_a_disagreement_of_the_pair_poisons_the_engine():
    dev = PairDevice(slots=5)
    eng, lib, h = _raw_engine(dev)
    a, b = torch.arange(10, 20), torch.arange(30, 38)
    dev.disagree_at = (2, a.numel() + 3)
    jc, ju = _join(a, 2, n_new=20), _join(b, 3)
    assert _submit_guided(lib, h, jc, ju) == 0
    rc, toks, _ = _read_all(lib, h, 2)
    assert rc != 0 and len(toks) == 3
    text = lib.dtk_engine_last_error(h).decode()
    assert "guided pair (2, 3)" in text, text
    j = _join(a, 0)
    assert lib.dtk_engine_join(h, C.byref(j)) != 0 and b"failed earlier" in j.error_out
    dev.bpending.clear()
    eng.close()


def test_a_failure_in_the_second_half_leaves_no_pair_and_both_slots_free():
    dev = PairDevice(slots=5)
    eng, lib, h = _raw_engine(dev)
    a, b = torch.arange(10, 20), torch.arange(30, 38)
    dev.fail_prefill_of = b.numel()
    jc, ju = _join(a, 0), _join(b, 1)
    assert _submit_guided(lib, h, jc, ju) != 0 and b"scripted prefill failure" in jc.error_out
    assert dev.pairs == {} and not [e for e in dev.log if e[0] == "set_guidance"]
    dev.fail_prefill_of = None
    for slot in (1, 0):         # the next unguided join into either slot steps alone
        n0 = len(dev.log)
        j = _join(a, slot, n_new=3)
        assert lib.dtk_engine_join(h, C.byref(j)) == 0
        assert _read_all(lib, h, slot)[0] == 0
        lib.dtk_engine_leave(h, slot)
        lib.dtk_engine_set_option(h, b"drain", 0)
        assert {e[1] for e in dev.log[n0:] if e[0] == "launch"} == {(slot,)}
    # bad arguments are refused in submit, with a text
    jc, ju = _join(a, 0), _join(b, 0)
    assert _submit_guided(lib, h, jc, ju) == ERR_STATE and b"distinct" in jc.error_out
    assert _submit_guided(lib, h, _join(a, 0), _join(b, 1), scale=1.0) == ERR_ARG
    eng.close()


def test_a_stale_pair_is_dissolved_before_its_slot_is_reused():
    dev = PairDevice(slots=5)
    eng, lib, h = _raw_engine(dev)
    a, b = torch.arange(10, 20), torch.arange(30, 38)
    jc, ju = _join(a, 0, n_new=2), _join(b, 1)
    assert _submit_guided(lib, h, jc, ju) == 0 and _read_all(lib, h, 0)[0] == 0
    lib.dtk_engine_leave(h, 0)
    lib.dtk_engine_set_option(h, b"drain", 0)
    assert dev.pairs == {0: (1, 2.0)}               # dissolving waits for the next join: a pair with neither slot active costs nothing
    n0 = len(dev.log)
    j = _join(a, 0, n_new=3)                        # the scripted device refuses half a pair, as the library does
    assert lib.dtk_engine_join(h, C.byref(j)) == 0, j.error_out
    assert _read_all(lib, h, 0)[0] == 0
    lib.dtk_engine_leave(h, 0)
    lib.dtk_engine_set_option(h, b"drain", 0)
    log = dev.log[n0:]
    assert log[0] == ("set_guidance", 0, None, 1.0) and dev.pairs == {}
    assert {e[1] for e in log if e[0] == "launch"} == {(0,)}
    # ... and so is one whose unconditional slot a guided join takes as its conditional one
    assert _submit_guided(lib, h, _join(a, 2, n_new=1), _join(b, 3)) == 0 and _read_all(lib, h, 2)[0] == 0
    lib.dtk_engine_leave(h, 2)
    lib.dtk_engine_set_option(h, b"drain", 0)
    assert _submit_guided(lib, h, _join(a, 3, n_new=1), _join(b, 1), scale=3.0) == 0 and _read_all(lib, h, 3)[0] == 0
    lib.dtk_engine_leave(h, 3)
    assert dev.pairs == {3: (1, 3.0)}
    eng.close()


def test_an_engine_without_the_op_refuses_in_submit():
    dev = PairDevice(slots=5)
    eng = NativeBatchEngine(dev, max_batch=4)       # guided_pairs=0: the op is not handed over
    a, b = torch.arange(10, 20), torch.arange(30, 38)
    jc, ju = _join(a, 0), _join(b, 1)
    assert _submit_guided(eng.lib, eng._h, jc, ju) == ERR_STATE and b"dtk_engine_set_guidance_op" in jc.error_out
    assert not dev.log or all(e[0] != "reserve_guidance" for e in dev.log)
    eng.close()


@ENGINES
def test_guided_pairs_zero_keeps_the_refusal(make):
    proc = fake_processor(VOCAB, NIMG)
    ids, px = prompt(proc, 0)
    dev = PairDevice(slots=5)
    eng = make(dev, max_batch=4)
    assert eng.guided_pairs == 0
    with pytest.raises(NotImplementedError, match="^guidance_scale: not in the batch engines yet"):
        _guided(dev, ids, px, torch.ones_like(px), 1, max_new_tokens=4)
    assert dev.log == []
    with pytest.raises(NotImplementedError, match="^guidance_scale: not in the batch engines yet"):
        with eng.sequence(ids, px, {}, guidance=dict(scale=2.0, ids=ids, pixel_values=px * 0)):
            pass
    eng.close()
    with pytest.raises(ValueError, match="guided_pairs"):
        make(PairDevice(slots=5), max_batch=4, guided_pairs=3)


@ENGINES
def test_guided_sequences_with_an_odd_number_of_slots_and_one_negative_encode(make):
    """five decode slots, four images, six threads: two guided sequences decode at once, a fifth slot serves the unguided ones; every
    sequence is what it is alone; the white negative image is encoded into the prefix cache once and forked into every pair"""
    proc = fake_processor(VOCAB, NIMG)
    white = None
    jobs = []
    for k in range(4):
        ids, px = prompt(proc, k, extra=[40 + k])
        white = torch.ones_like(px) if white is None else white
        jobs.append((ids, px, 100 + k))
    kw = dict(max_new_tokens=14)
    alone = [_alone(i, p, white, s, 1.5 + 0.5 * k, **kw) for k, (i, p, s) in enumerate(jobs)]
    plain_dev = PairDevice()
    plain = [plain_dev.generate(input_ids=i[None], pixel_values=p, seed=s, **KW, **kw) for i, p, s in jobs]
    dev = PairDevice(slots=17)
    eng = make(dev, max_batch=5, guided_pairs=2)
    got, got_plain = [None] * 4, [None] * 4

    def worker(k):
        if k < 4:
            i, p, s = jobs[k]
            got[k] = _guided(dev, i, p, white, s, 1.5 + 0.5 * k, owner=k, **kw)
        else:
            for n in range(k - 4, 4, 2):
                i, p, s = jobs[n]
                got_plain[n] = dev.generate(input_ids=i[None], pixel_values=p, seed=s, **KW, **kw)
    threads(6, worker)
    eng.close()          # (the Python-driven engine frees the slots of a last speculative step when that step is collected)
    st = eng.stats()
    assert sorted(eng.free) == [0, 1, 2, 3, 4]
    for k in range(4):
        assert torch.equal(got[k], alone[k]), k
        assert torch.equal(got_plain[k], plain[k]), k
    assert st["prefix_encodes"] == 5                # four images and the one white canvas
    steps = [e[1] for e in dev.log if e[0] == "launch"]
    sets = [e for e in dev.log if e[0] == "set_guidance" and e[2] is not None]
    assert len(sets) == 4
    assert dev.pairs == {} and all(len(s) <= 5 for s in steps)


@pytest.mark.parametrize("which", ["native", "python"])
def test_simulate_parallel_with_guidance_end_to_end(which, monkeypatch):
    """three guided trees over a 9-slot scripted device: every rollout arrives, never more than decode_slots // 2 pairs decode at
    once, no step holds half a pair (the device asserts it), no pair and no held slot is left; the search is reproducible"""
    from detikzify_amd.infer import DetikzifyPipeline, SyntheticTikzDocument
    from detikzify_amd.infer.batching import simulate_parallel
    from .helpers import sketch_image
    monkeypatch.setenv("DTK_ENGINE", which)
    proc = fake_processor(VOCAB, NIMG)
    image = sketch_image(5, 96)

    def run(slots, trees=3):
        dev = PairDevice(slots=slots)
        pipe = DetikzifyPipeline(dev, proc, metric="fast", document_class=SyntheticTikzDocument, max_length=NIMG + 40, compile_timeout=None)
        res = sorted((doc.code, score) for score, doc in simulate_parallel(pipe, image, trees=trees, expansions_per_tree=2, guidance_scale=2.0))
        assert dev.batch_engine is None and dev.pairs == {} and not dev.bpending
        assert dev.last_batch_stats["engine"] == which
        return res, dev

    res, dev = run(9)
    assert len(res) == 6
    assert ("reserve_guidance", 3) in dev.log and dev.log[-1] == ("reserve_guidance", 0)
    steps = [e[1] for e in dev.log if e[0] == "launch"]
    assert steps and max(len(s) for s in steps) <= 6 and all(len(s) % 2 == 0 for s in steps)
    assert dev.last_batch_stats["prefix_encodes"] == 2          # the image and the white canvas, once each
    assert run(9)[0] == res
    # five decode-capable slots... of a 5-slot device four decode: two pairs at a time, the third tree takes its turn
    crowded, dev5 = run(5)
    assert ("reserve_guidance", 2) in dev5.log and max(len(e[1]) for e in dev5.log if e[0] == "launch") <= 4
    assert len(crowded) == 6
