"""
NativeBatchEngine — the batch of rollouts of one GPU, driven by the native run loop of libdtk_hip.so (include/dtk.h,
"dtk_engine_*"; csrc/dtk_engine.cpp).

Same contract as infer/batching.BatchEngine (the Python-driven engine it replaces as the default): every rollout is a thread
inside `model.generate` (reference detikzify/infer/generate.py:246-282 runs it in a worker thread and consumes the stream line by
line), and all of them share one pass over the weights per decode step.  What changed is who turns the crank: a native thread
launches and collects the steps (two in flight), keeps every slot's tokens in a ring and applies the sequence's stop rules (EOS,
max_length); the rollout threads block in dtk_engine_read — outside the interpreter lock — and wake once per source line, not once
per token.  Python keeps what is policy: which slot a sequence gets, which slot still holds which image prefix (fork / in-place
reuse / prefix-cache LRU), and what each join therefore has to do; the native loop executes the joins in the order they were
planned.  A slot's arithmetic does not depend on its company, so a sequence is the same tokens as under BatchEngine (tests).

Text-conditioned sequences (the TikZero adapter: sequence(text_ids=...), dtk_engine_submit_text) share the slots with image-only
ones.  Their prefix identity is (image key, text key, prefix length) — text key 0 for image-only prompts, DUMMY_IMAGE_KEY for a
text without an image — so a prefix is forked or reused in place only under the same image AND text.
"""
from __future__ import annotations

import ctypes as C
import threading
from collections import OrderedDict
from contextlib import contextmanager
from typing import Any, Callable, Dict, Iterable, Iterator, List, Optional, Tuple

import torch

from .. import _lib


class _NativeSequence:
    def __init__(self, engine: "NativeBatchEngine", slot: int, logprobs: bool = False, top: int = 0):
        self.engine, self.slot = engine, slot
        # sequence(logprobs=True, top_logprobs=j): per token read so far its j most likely tokens and their log-probabilities
        # (dtk_engine_read_top; the engine's own k >= j columns are cut to j)
        self._top = int(top)
        self.top_ids: Optional[List[List[int]]] = [] if top else None
        self.top_logprobs: Optional[List[List[float]]] = [] if top else None
        self._ti, self._tl = ((C.c_int32 * (256 * _lib.DTK_MAX_TOP))(), (C.c_float * (256 * _lib.DTK_MAX_TOP))()) if top else (None, None)
        self._buf = (C.c_int64 * 256)()
        # sequence(logprobs=True): the (logprob, sample_logprob) of every token read so far, in token order (dtk_engine_read_lp)
        self.logprobs: Optional[List[float]] = [] if logprobs else None
        self.sample_logprobs: Optional[List[float]] = [] if logprobs else None
        self._lp, self._slp = ((C.c_float * 256)(), (C.c_float * 256)()) if logprobs else (None, None)
        self._n, self._state = C.c_int32(0), C.c_int32(0)
        self._pending: List[int] = []
        self.ended = False

    def _read(self, cap: int, timeout_ms: int) -> List[int]:
        e = self.engine
        if self._top:
            rc = e.lib.dtk_engine_read_top(e._h, self.slot, self._buf, self._lp, self._slp, self._ti, self._tl, cap, C.byref(self._n),
                                           C.byref(self._state), timeout_ms)
            if rc == 0 and self._n.value:
                self.logprobs.extend(self._lp[:self._n.value])
                self.sample_logprobs.extend(self._slp[:self._n.value])
                for i in range(self._n.value):
                    at = i * _lib.DTK_MAX_TOP
                    self.top_ids.append(list(self._ti[at:at + self._top]))
                    self.top_logprobs.append(list(self._tl[at:at + self._top]))
        elif self.logprobs is not None:
            rc = e.lib.dtk_engine_read_lp(e._h, self.slot, self._buf, self._lp, self._slp, cap, C.byref(self._n), C.byref(self._state), timeout_ms)
            if rc == 0 and self._n.value:
                self.logprobs.extend(self._lp[:self._n.value])
                self.sample_logprobs.extend(self._slp[:self._n.value])
        else:
            rc = e.lib.dtk_engine_read(e._h, self.slot, self._buf, cap, C.byref(self._n), C.byref(self._state), timeout_ms)
        if rc != 0:
            raise _lib.DtkError(f"the batch engine's device failed ({rc}): {e.lib.dtk_engine_last_error(e._h).decode(errors='replace')}")
        n = self._n.value
        if self._state.value != _lib.DTK_SEQ_RUNNING:
            self.ended = True
        return self._buf[:n] if n else []

    def run(self, emit: Callable[[int], bool]):
        """`emit.many(tokens) -> stop` (or emit(token) per token) for every burst of this sequence's tokens, in this thread; returns
        when emit asked to stop, or the sequence ended by its own rules (stop id, token budget)."""
        many = getattr(emit, "many", None)
        aborted = getattr(emit, "aborted", None)
        while True:
            toks = self._read(256, 100)
            if toks:
                if many is not None:
                    if many(toks):
                        return
                else:
                    for tok in toks:
                        if emit(tok):
                            return
            elif aborted is not None and aborted():       # nothing new for 100 ms (a join's prefill, a paused batch): poll the flag
                return
            if self.ended:
                return

    def next_token(self) -> int:
        """pull: the next token of this sequence (blocks); a sequence that has ended raises StopIteration"""
        while True:
            if self._pending:
                return self._pending.pop(0)
            if self.ended:
                raise StopIteration
            self._pending = list(self._read(256, -1))


class _ScriptedOps:
    """dtk_engine_ops over a Python model object (the CPU tests' scripted device): the native loop calls back into Python for every
    device operation.  Exceptions become error codes; an AssertionError (a scripted device's protocol check) stops the engine."""

    def __init__(self, model, engine: "NativeBatchEngine"):
        self.model, self.engine = model, engine
        self._err = C.create_string_buffer(512)     # the text last_error hands to the native side (owned here)
        O = _lib.DtkEngineOps

        def guard(f):
            def g(*a):
                try:
                    r = f(*a)
                    return 0 if r is None else r
                except AssertionError as e:
                    self._err.value = f"scripted device: {e!r}".encode()[:511]
                    return -2
                except BaseException as e:  # noqa: BLE001
                    self._err.value = str(e).encode()[:511]
                    return -1
            return g

        def ids_of(ptr, n):
            return torch.tensor([ptr[i] for i in range(n)], dtype=torch.int64)

        def launch(dev, active):
            model.decode_batch_launch([j for j in range(_lib.DTK_MAX_BATCH) if active[j]])

        def wait(dev, out):
            toks = model.decode_batch_wait()
            for j in range(_lib.DTK_MAX_BATCH):
                out[j] = toks[j]

        def wait_lp(dev, out, lp_out, slp_out):
            toks, lp, slp = model.decode_batch_wait_lp()
            for j in range(_lib.DTK_MAX_BATCH):
                out[j], lp_out[j], slp_out[j] = toks[j], lp[j], slp[j]

        def wait_top(dev, out, lp_out, slp_out, ti_out, tl_out):
            toks, lp, slp, ti, tl = model.decode_batch_wait(top=True)
            for j in range(_lib.DTK_MAX_BATCH):
                out[j], lp_out[j], slp_out[j] = toks[j], lp[j], slp[j]
                for i in range(_lib.DTK_MAX_TOP):
                    has = i < len(ti[j])
                    ti_out[j * _lib.DTK_MAX_TOP + i] = ti[j][i] if has else -1
                    tl_out[j * _lib.DTK_MAX_TOP + i] = tl[j][i] if has else float("nan")

        def prefill(dev, slot, ids, T, pixels, key, flags):
            px = engine._pixels_by_key.get(int(key)) if pixels else None
            model.prefill(ids_of(ids, T), px, slot=slot, reuse=bool(flags & _lib.DTK_PREFILL_REUSE_PREFIX))

        def prefill_text(dev, slot, ids, T, pixels, key, tids, n_text, tkey, flags):
            px = engine._pixels_by_key.get(int(key)) if pixels else None
            model.prefill(ids_of(ids, T), px, slot=slot, reuse=bool(flags & _lib.DTK_PREFILL_REUSE_PREFIX), adapter_input_ids=ids_of(tids, n_text))

        def sampling(dev, slot, sp):
            s = sp.contents
            model.set_sampling(slot=slot, do_sample=bool(s.do_sample), temperature=s.temperature, top_p=s.top_p, top_k=s.top_k, seed=s.seed,
                               bad_ids=list(s.bad_ids[:s.n_bad]), begin_suppress_ids=list(s.begin_suppress_ids[:s.n_begin_suppress]),
                               always_suppress_ids=list(s.always_suppress_ids[:s.n_always_suppress]))

        def sampling_ext(dev, slot, xp):
            model.set_sampling_ext(float(xp.contents.min_p), float(xp.contents.epsilon_cutoff), slot=slot)

        def penalties(dev, slot, presence, frequency, start):
            model.set_penalties(float(presence), float(frequency), int(start), slot=slot)

        def dry(dev, slot, dp):
            d = dp.contents
            model.set_dry(float(d.multiplier), float(d.base), int(d.allowed_length), int(d.start),
                          tuple(int(d.breakers[i]) for i in range(int(d.n_breakers))), slot=slot)

        def length_control(dev, slot, lp):
            l = lp.contents
            model.set_length_control(int(l.min_new_tokens), (int(l.decay_start), float(l.decay_factor)) if l.decay_factor else None, int(l.start),
                                     tuple(int(l.eos_ids[i]) for i in range(int(l.n_eos))), slot=slot)

        def logit_bias(dev, slot, ids, values, n):
            model.set_logit_bias(tuple((int(ids[i]), float(values[i])) for i in range(int(n))), slot=slot)

        def guidance(dev, cond, uncond, scale):
            model.set_guidance(float(scale), int(cond), int(uncond) if uncond >= 0 else None)

        def fork(dev, a, b, n):
            model.kv_fork(a, b, n)

        def lcp(dev, slot, ids, n, key, out):
            best = model.best_lcp_slot([slot], ids_of(ids, n), int(key))
            out[0] = best[1] if best else 0

        def resume(dev, slot, ids, n, key):
            model.resume_slot(slot, ids_of(ids, n), int(key))

        def ctxlen(dev, slot):
            return int(model.lib.dtk_context_len_slot(model._ctx, slot))

        def lasterr(dev):
            return C.addressof(self._err)

        self.keep = [O.LAUNCH(guard(launch)), O.WAIT(guard(wait)), O.PREFILL(guard(prefill)), O.SAMPLING(guard(sampling)), O.FORK(guard(fork)),
                     O.LCP(guard(lcp)), O.RESUME(guard(resume)), O.CTXLEN(ctxlen), O.LASTERR(lasterr)]
        self.ops = O(None, *self.keep, int(model.config.max_positions), int(engine.decode_slots))
        # the text prefill only for a device that has an adapter (an engine without it refuses text joins in submit)
        self.prefill_text = O.PREFILL_TEXT(guard(prefill_text)) if _has_adapter(model) else None
        self.wait_lp = O.WAIT_LP(guard(wait_lp))       # handed to the engine by the first sequence(logprobs=True)
        self.wait_top = O.WAIT_TOP(guard(wait_top))    # handed to an engine built with top_logprobs=k
        self.sampling_ext = O.SAMPLING_EXT(guard(sampling_ext)) if hasattr(model, "set_sampling_ext") else None
        self.penalties = O.PENALTIES(guard(penalties)) if hasattr(model, "set_penalties") else None
        self.dry = O.DRY(guard(dry)) if hasattr(model, "set_dry") else None
        self.length_control = O.LENGTH_CTL(guard(length_control)) if hasattr(model, "set_length_control") else None
        self.logit_bias = O.LOGIT_BIAS(guard(logit_bias)) if hasattr(model, "set_logit_bias") else None
        self.guidance = O.GUIDANCE(guard(guidance)) if hasattr(model, "set_guidance") else None


def _has_adapter(model) -> bool:
    probe = getattr(model, "has_adapter", None)
    return bool(probe()) if callable(probe) else False


class NativeBatchEngine:
    """One engine per model; every method is thread-safe.  `sequence()` is the per-rollout entry (model.generate uses it when
    model.batch_engine is set): plan the join under the engine's lock, queue it natively in plan order, wait for it outside the lock."""
    native = True

    def __init__(self, model, max_batch: Optional[int] = None, share_prefix: bool = True, pipeline: bool = True, gather: int = 0,
                 gather_timeout: float = 0.5, prefix_slots: Optional[int] = None, resume_in_place: bool = True,
                 flush_tokens: Optional[Iterable[int]] = None, flush_max: int = 32, guided_pairs: int = 0,
                 top_logprobs: Optional[int] = None):
        """`top_logprobs`=k (1 .. 8): every step of this engine also delivers the k most likely tokens of the logits each token was sampled
        from; sequence(logprobs=True, top_logprobs=j <= k) collects them.  The constructor switches the model over (enable_logprobs() +
        enable_top_logprobs(k)) before any join, close() restores what it found.  The switches refuse unread single-sequence steps, and a
        plain generate() usually leaves one behind, so the constructor first resets the model's single-sequence sampling state
        (model.set_sampling(): default greedy sampling, unread steps forgotten); close() does not bring that back — every generate() sets
        its own.  None (the default): sequences that ask are refused.
        `guided_pairs`=P > 0: up to P classifier-free-guided sequences (sequence(guidance=...), model.generate's guidance_scale)
        decode at once, each in two slots; the device's pair table is reserved for P standing pairs (model.reserve_guidance), so a
        pair that forms or dissolves re-captures nothing.  0 (the default): nothing is reserved and guided sequences are refused."""
        from ..model.modeling import check_top_logprobs
        self.top_logprobs = check_top_logprobs(top_logprobs)
        n = model.num_slots()
        if n <= 0:
            raise ValueError("model was loaded without batch slots (load(..., batch_slots=N))")
        self.model = model
        self.lib = _lib.load_library()
        probe = getattr(model, "max_decode_slots", None)
        dec = int(probe()) if callable(probe) else min(n, 64 if n > 33 else (32 if n > 17 else 16))
        self.decode_slots = dec
        self.share_prefix = share_prefix and n >= 2
        self.capacity = min(dec, max_batch) if max_batch else (dec if n > dec else dec - 1)
        self.guided_pairs = int(guided_pairs)
        if self.guided_pairs < 0 or 2 * self.guided_pairs > self.capacity:
            raise ValueError(f"guided_pairs = {guided_pairs}: every guided sequence takes two of the engine's {self.capacity} decode slots")
        spare = n - self.capacity       # slots the decode batch does not need hold image prefixes (see BatchEngine)
        n_prefix = min(spare, 8 if prefix_slots is None else int(prefix_slots)) if self.share_prefix else 0
        self.prefix_slots: List[int] = list(range(n - n_prefix, n))
        self.prefix_cache: "OrderedDict[Tuple[int, int, int], int]" = OrderedDict()    # (image key, text key, prefix length) -> slot
        self.slot_img: Dict[int, Tuple[int, int, int]] = {}
        self._adapter_epoch = getattr(model, "adapter_epoch", 0)
        self.resume_in_place = resume_in_place
        self.last_slot: Dict[int, int] = {}
        self.joins = self.resumes = self.inplace_reuses = self.prefix_encodes = 0
        self.flush_max = int(flush_max)
        self._cv = threading.Condition()        # protects the bookkeeping above and `free`; joins are queued natively under it
        self.free: List[int] = list(range(self.capacity))
        self._pixels_by_key: Dict[int, Any] = {}
        self._lp = False                        # the device's steps deliver log-probabilities (first sequence(logprobs=True))
        self._h = C.c_void_p()
        ctx = getattr(model, "_ctx", None)
        if ctx:
            rc = self.lib.dtk_engine_create(ctx, C.byref(self._h))
            self._scripted = None
        else:
            self._scripted = _ScriptedOps(model, self)
            rc = self.lib.dtk_engine_create_ops(C.byref(self._scripted.ops), C.byref(self._h))
            if rc == 0 and self._scripted.prefill_text is not None and hasattr(self.lib, "dtk_engine_set_prefill_text_op"):
                rc = self.lib.dtk_engine_set_prefill_text_op(self._h, self._scripted.prefill_text)
            if rc == 0 and self._scripted.sampling_ext is not None:
                rc = self.lib.dtk_engine_set_sampling_ext_op(self._h, self._scripted.sampling_ext)
            if rc == 0 and self._scripted.penalties is not None:
                rc = self.lib.dtk_engine_set_penalties_op(self._h, self._scripted.penalties)
            if rc == 0 and self._scripted.dry is not None and hasattr(self.lib, "dtk_engine_set_dry_op"):
                rc = self.lib.dtk_engine_set_dry_op(self._h, self._scripted.dry)
            if rc == 0 and self._scripted.length_control is not None and hasattr(self.lib, "dtk_engine_set_length_control_op"):
                rc = self.lib.dtk_engine_set_length_control_op(self._h, self._scripted.length_control)
            if rc == 0 and self._scripted.logit_bias is not None and hasattr(self.lib, "dtk_engine_set_logit_bias_op"):
                rc = self.lib.dtk_engine_set_logit_bias_op(self._h, self._scripted.logit_bias)
            if rc == 0 and self.guided_pairs and self._scripted.guidance is not None:
                rc = self.lib.dtk_engine_set_guidance_op(self._h, self._scripted.guidance)
        if rc != 0:
            raise _lib.DtkError(f"dtk_engine_create failed ({rc})")
        self._found_options = None
        if self.top_logprobs:
            try:        # no sequence has joined: the switches' own refusals (unread single-sequence steps, another engine's sequences) hold
                self._found_options = (model.logprobs_enabled, model.top_logprobs_enabled)
                model.set_sampling()        # the single sequence starts afresh: see the constructor's docstring / comment on top_logprobs
                model.enable_top_logprobs(self.top_logprobs)
                if self._scripted is not None and self.lib.dtk_engine_set_wait_top_op(self._h, self._scripted.wait_top) != 0:
                    raise _lib.DtkError("dtk_engine_set_wait_top_op failed")
                self._lp = True
            except BaseException:
                self._restore_options()
                self.lib.dtk_engine_destroy(self._h)
                self._h = C.c_void_p()
                raise
        if self.guided_pairs:
            try:
                model.reserve_guidance(self.guided_pairs)
            except BaseException:
                self._restore_options()
                self.lib.dtk_engine_destroy(self._h)
                self._h = C.c_void_p()
                raise
        if not pipeline:
            self.lib.dtk_engine_set_option(self._h, b"depth", 1)
        self.has_flush_tokens = False
        if flush_tokens is not None:
            self.set_flush_tokens(flush_tokens)
        if gather:
            self.expect(gather, gather_timeout)
        model.batch_engine = self

    # ---- configuration -------------------------------------------------------------------------------------------------------
    def set_flush_tokens(self, token_ids: Iterable[int]):
        ids = sorted({int(t) for t in token_ids})
        arr = (C.c_int64 * max(1, len(ids)))(*ids)
        if self.lib.dtk_engine_set_flush_tokens(self._h, arr, len(ids)) != 0:
            raise _lib.DtkError("dtk_engine_set_flush_tokens failed")
        self.has_flush_tokens = bool(ids)

    def expect(self, n: int, timeout: float = 0.5):
        self.lib.dtk_engine_expect(self._h, int(n), int(timeout * 1000))

    def native_stats(self) -> Dict[str, Any]:
        st = _lib.DtkEngineStats()
        self.lib.dtk_engine_get_stats(self._h, C.byref(st))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def stats(self) -> Dict[str, Any]:
        st = self.native_stats() if self._h else self._final
        return {"engine": "native", "steps": st["steps"], "tokens_out": st["tokens_out"], "wait_s": round(st["wait_s"], 3),
                "launch_s": round(st["launch_s"], 3), "prefill_s": round(st["join_s"], 3), "drain_s": round(st["drain_s"], 3),
                "host_bound_steps": st["host_bound_steps"], "prefix_encodes": self.prefix_encodes, "inplace_reuses": self.inplace_reuses,
                "joins": self.joins, "resumed_in_place": self.resumes, "idle_between_steps_s": round(st["idle_s"], 3),
                "steps_below_half_occupancy": st["steps_below_half_occupancy"], "reader_wakeups": st["reader_wakeups"],
                "wasted_slot_steps": st["wasted_slot_steps"],
                "span_s": round(st["last_collect_t"] - st["first_launch_t"], 3) if st["first_launch_t"] else 0.0}

    def close(self):
        if self._h:
            self._final = self.native_stats()
            h, self._h = self._h, C.c_void_p()
            self.lib.dtk_engine_destroy(h)
            if self.guided_pairs:       # the loop has stopped, no step is in flight: the pairs it left and the reservation go
                for slot in range(self.decode_slots):
                    g = self.model.guidance(slot)
                    if g is not None and g["is_cond"]:
                        self.model.set_guidance(None, slot, None)
                self.model.reserve_guidance(0)
            self._restore_options()
        if getattr(self.model, "batch_engine", None) is self:
            self.model.batch_engine = None

    def _restore_options(self):
        """top_logprobs=k: the model's two options as the constructor found them (the loop has stopped: nothing is in flight)"""
        if self._found_options is not None:
            (lp, k), self._found_options = self._found_options, None
            self.model.enable_top_logprobs(k)
            if not lp:
                self.model.disable_logprobs()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def prefix_slot(self) -> Optional[int]:
        return self.prefix_slots[-1] if self.prefix_slots else None

    @property
    def steps(self) -> int:
        return int((self.native_stats() if self._h else self._final)["steps"])

    def busy(self) -> bool:
        """some sequence holds a slot (joined, or being joined)"""
        with self._cv:
            return len(self.free) < self.capacity

    def _enable_logprobs(self):
        """(under _cv, no sequence holding a slot) the device's steps deliver log-probabilities from here on"""
        if not self.model.logprobs_enabled:
            # the native loop may still be collecting the last steps behind sequences that have just left: wait until none is in flight
            if self.lib.dtk_engine_set_option(self._h, b"drain", 0) != 0:
                raise _lib.DtkError("dtk_engine_set_option(drain) failed")
            self.model.enable_logprobs()
        if self._scripted is not None and self.lib.dtk_engine_set_wait_lp_op(self._h, self._scripted.wait_lp) != 0:
            raise _lib.DtkError("dtk_engine_set_wait_lp_op failed")
        self._lp = True

    # ---- joins ---------------------------------------------------------------------------------------------------------------
    def _prefix_key(self, ids, image_key: int, text_key: int):
        """(image key, text key, prefix length) if the prompt starts with its image-token run, else None"""
        tok = self.model.config.image_token_id
        ids = ids.reshape(-1)
        n_img = int((ids == tok).sum())
        if n_img == 0 or not bool((ids[:n_img] == tok).all()):
            return None
        return (image_key, text_key, n_img)

    def _check_adapter_epoch(self):
        """(under _cv) creating or unloading the adapter clears every slot's cached ids on the C side: forget what the bookkeeping
        says the slots hold"""
        epoch = getattr(self.model, "adapter_epoch", 0)
        if epoch != self._adapter_epoch:
            self._adapter_epoch = epoch
            self.prefix_cache.clear()
            self.slot_img.clear()

    def _plan_prefix(self, j: "_lib.DtkJoin", slot: int, key) -> Callable[[], None]:
        """what a join of an image prompt into `slot` has to do to get the image prefix there (BatchEngine._fork_prefix, as a plan):
        fills j's prefix fields, returns the bookkeeping to apply once the plan is certain to run.  Sources, in order: a prefix-cache
        slot that holds this image (its fork also carries the logits); the slot itself (in place); any other slot that still holds
        the prefix (donor); else the image is encoded into a free — else the least recently used — prefix-cache slot."""
        n_img = key[2]
        j.prefix_len = n_img
        src = self.prefix_cache.get(key)
        if src is None and self.slot_img.get(slot) == key:
            j.prefix_in_place = 1
            return lambda: None
        if src is not None:
            j.prefix_src, j.prefix_src_whole = src, 1

            def apply_cached():
                self.slot_img[slot] = key
                self.prefix_cache.move_to_end(key)
            return apply_cached
        donor = next((s for s, k in self.slot_img.items() if k == key and s != slot), None)
        if donor is not None:
            j.prefix_src, j.prefix_src_whole = donor, 0
            return lambda: self.slot_img.__setitem__(slot, key)
        if not self.prefix_slots:       # nobody holds this image and there is no prefix-cache slot: full prefill, the slot becomes a donor
            j.prefix_len = 0

            def apply_full():
                self.slot_img[slot] = key
                self.prefix_encodes += 1
            return apply_full
        used = set(self.prefix_cache.values())
        src = next((s for s in reversed(self.prefix_slots) if s not in used), None)
        evict = None
        if src is None:
            evict, src = next(iter(self.prefix_cache.items()))      # least recently used image
        j.prefix_src, j.prefix_src_whole, j.prefix_encode = src, 1, 1

        def apply_encode():
            if evict is not None:
                self.prefix_cache.pop(evict, None)
            self.prefix_cache[key] = src
            self.prefix_cache.move_to_end(key)
            self.slot_img[slot] = key
            self.prefix_encodes += 1
        return apply_encode

    @contextmanager
    def sequence(self, ids, pixel_values, sampling: Dict[str, Any], owner: Optional[int] = None, max_new_tokens: Optional[int] = None,
                 stop_ids: Iterable[int] = (), per_token: bool = True, text_ids=None, logprobs: bool = False,
                 top_logprobs: Optional[int] = None, guidance: Optional[Dict[str, Any]] = None) -> Iterator[_NativeSequence]:
        """`owner`: see BatchEngine.sequence.  `max_new_tokens` / `stop_ids`: the sequence's own end (the native loop stops it there);
        `per_token`: the reader is woken for every token (arbitrary stopping criteria / foreign streamers) instead of per line.
        `text_ids`: one unpadded text that conditions the tower (the adapter); pixel_values may then be None (the dummy image).
        `logprobs`: the sequence collects its tokens' (logprob, sample_logprob) in `.logprobs` / `.sample_logprobs`.  The first such
        sequence switches the device over, which needs every slot free: ask for it before other sequences join (or call
        model.enable_logprobs() before the engine is built).
        `guidance`: dict(scale=, ids=, pixel_values=, text_ids=) — a classifier-free-guided sequence (an engine built with
        guided_pairs > 0): the negative branch (its prompt, image and / or text) decodes in a second slot of its own, planned like the
        sequence's — its own prefix key, so one negative image is encoded once and forked into every guided sequence's second slot, its
        own slot per owner for resume — and both slots are released together.  `sampling`, `max_new_tokens` and `stop_ids` describe the
        sequence; the second slot samples nothing of its own."""
        top = self._check_top(top_logprobs, logprobs)
        if not self._h:
            raise _lib.DtkError("the batch engine is closed")
        if guidance is not None and not self.guided_pairs:
            raise NotImplementedError("guidance_scale: not in the batch engines yet (this engine was built without guided_pairs=)")
        from ..model.modeling import DUMMY_IMAGE_KEY, adapter_text, check_guidance_scale, text_key

        def plan_of(ids, pixel_values, text_ids):
            """the part of a join that is the prompt's own: (join, prefix key, the tensors it points into)"""
            ids = ids.detach().to("cpu", torch.int64).reshape(-1).contiguous()
            tids = adapter_text(text_ids) if text_ids is not None else None
            tkey = text_key(tids) if tids is not None else 0
            if tids is not None and not hasattr(self.lib, "dtk_engine_submit_text"):
                raise _lib.DtkError("this library has no dtk_engine_submit_text: text-conditioned sequences cannot join the batch")
            ikey = self.model.image_key(pixel_values) if pixel_values is not None else (DUMMY_IMAGE_KEY if tids is not None else 0)
            want = self._prefix_key(ids, ikey, tkey) if (self.share_prefix and (pixel_values is not None or tids is not None)) else None
            px = None
            if pixel_values is not None:
                px = pixel_values.detach().to("cpu", torch.float32).contiguous()
                if px.dim() == 4:
                    if px.shape[0] != 1:
                        raise ValueError("batch size 1 only")
                    px = px[0]
            j = _lib.DtkJoin()
            j.n_ids, j.ids = int(ids.numel()), ids.data_ptr()
            j.pixels = px.data_ptr() if px is not None else None
            j.image_key = ikey
            j.prefix_src = -1
            j.full_flags = (_lib.DTK_PREFILL_REUSE_PREFIX | _lib.DTK_PREFILL_REUSE_IMAGE) if getattr(self.model, "reuse_prefix", False) else 0
            if self._scripted is not None and pixel_values is not None:
                self._pixels_by_key[int(ikey)] = pixel_values
            return j, want, ids, px, tids, tkey

        j, want, ids, px, tids, tkey = plan_of(ids, pixel_values, text_ids)
        n_ids = int(ids.numel())
        gj = gwant = gids = gpx = gtids = None
        gtkey, gscale = 0, 1.0
        if guidance is not None:
            gscale = check_guidance_scale(guidance.get("scale"))
            if gscale == 1.0:
                raise ValueError("sequence(guidance=...): a scale of 1 is no guidance")
            g_in = guidance.get("ids")
            gj, gwant, gids, gpx, gtids, gtkey = plan_of(ids if g_in is None else g_in, guidance.get("pixel_values"), guidance.get("text_ids"))
        s = j.sampling
        s.do_sample, s.temperature = int(bool(sampling.get("do_sample", False))), float(sampling.get("temperature", 1.0))
        s.top_p, s.top_k = float(sampling.get("top_p", 1.0)), int(sampling.get("top_k", 0) or 0)
        s.seed = int(sampling.get("seed", 0)) & ((1 << 64) - 1)
        for field, cnt, name in (("bad_ids", "n_bad", "bad_ids"), ("begin_suppress_ids", "n_begin_suppress", "begin_suppress_ids"),
                                 ("always_suppress_ids", "n_always_suppress", "always_suppress_ids")):
            vals = [int(v) for v in (sampling.get(name) or ())]
            if len(vals) > 8:
                raise ValueError("at most 8 ids per suppression list")
            setattr(s, cnt, len(vals))
            arr = getattr(s, field)
            for i, v in enumerate(vals):
                arr[i] = v
        from ..model.modeling import DRY_KEYS, check_dry, check_penalties, check_truncation, dry_struct, length_struct, shape_of_sampling
        ext = _lib.DtkSamplingExt(*check_truncation(sampling.get("min_p"), sampling.get("epsilon_cutoff")))
        has_ext = bool(ext.min_p or ext.epsilon_cutoff)
        pen_p, pen_f, pen_s = check_penalties(sampling.get("presence_penalty"), sampling.get("frequency_penalty"), sampling.get("penalty_start"))
        has_pen = bool(pen_p or pen_f)
        pen_s = (n_ids if pen_s is None else pen_s) if has_pen else 0      # penalty_start: the prompt length unless the sequence says otherwise
        dry_m, dry_b, dry_a, dry_s, dry_brk = check_dry(*(sampling.get(k) for k in DRY_KEYS))
        has_dry = bool(dry_m)
        dry = dry_struct(dry_m, dry_b, dry_a, (n_ids if dry_s is None else dry_s) if has_dry else 0, dry_brk)      # dry_start as penalty_start
        if has_dry and not hasattr(self.lib, "dtk_engine_submit_dry"):
            raise _lib.DtkError("this device takes no DRY penalty")
        # the length rules and the bias pairs (length_start as penalty_start)
        len_m, len_d, len_s, len_eos, bias_pairs = shape_of_sampling(sampling, n_ids)
        has_shape = bool(len_eos or bias_pairs)
        lctl = length_struct(len_m, len_d, len_s, len_eos)
        bias_ids = (C.c_int32 * max(len(bias_pairs), 1))(*[t for t, _ in bias_pairs])
        bias_val = (C.c_float * max(len(bias_pairs), 1))(*[v for _, v in bias_pairs])
        if has_shape and not hasattr(self.lib, "dtk_engine_submit_shape"):
            raise _lib.DtkError("this device takes no length control / logit bias")
        stops = [int(t) for t in stop_ids if int(t) >= 0][:8]
        j.n_stop = len(stops)
        for i, t in enumerate(stops):
            j.stop_ids[i] = t
        j.max_new_tokens = int(max_new_tokens) if max_new_tokens is not None else (1 << 30)
        j.flush_mode = 0 if per_token else 1
        j.flush_max = self.flush_max

        def pick(j, want, n_ids, last_tok, has_px, order, okey, cands_ok):
            """(under _cv) the slot of one prompt among the free slots `order` and where it may resume: fills j.slot / j.try_resume"""
            # resume in place: the prompt (all but its last token) is still in a free slot's cache — an MCTS tree coming back to a
            # node of its own previous rollout.  Whether that holds is decided by the native loop when the join executes
            # (dtk_slot_lcp behind every step in flight); the plan here only names where to look.  An owner looks in the slot IT used
            # last (so that resume-or-prefill never depends on which other slots happen to be free: BatchEngine.sequence).
            slot, cands = None, []
            may_resume = (self.resume_in_place and n_ids >= 2 and (want is not None or not has_px)
                          and last_tok != self.model.config.image_token_id)
            holds = (lambda f: self.slot_img.get(f) == want) if want is not None else (lambda f: f not in self.slot_img)
            if may_resume and okey is not None:
                last = self.last_slot.get(okey)
                if last in order and holds(last):
                    slot, j.try_resume = last, 1
            elif may_resume and cands_ok:
                cands = [f for f in order if holds(f)]
            if slot is None and okey is not None and self.last_slot.get(okey) in order:
                slot = self.last_slot[okey]
            if slot is None:
                slot = next((f for f in order if f not in self.slot_img), None)
            if slot is None and want is not None:
                slot = next((f for f in order if self.slot_img.get(f) == want), None)
            if slot is None:
                slot = order[0]
            j.slot = slot
            if okey is not None:
                self.last_slot[okey] = slot
            return slot, cands

        ticket = C.c_uint64(0)
        held_through = False
        if guidance is not None:
            cond = dict(j=j, want=want, ids=ids, tids=tids, tkey=tkey, has_px=pixel_values is not None, keep=px)
            neg = dict(j=gj, want=gwant, ids=gids, tids=gtids, tkey=gtkey, has_px=guidance.get("pixel_values") is not None, keep=gpx)
            tables = dict(ext=ext, pen=(pen_p, pen_f, pen_s), dry=dry, lctl=lctl, bias=(bias_ids, bias_val, len(bias_pairs)))
            yield from self._guided(cond, neg, gscale, owner, logprobs, tables, pick, top)
            return
        with self._cv:
            if logprobs:
                self._want_logprobs()
            while not self.free:
                self._cv.wait()
            order = sorted(self.free)
            self._check_adapter_epoch()
            slot, cands = pick(j, want, n_ids, int(ids[-1]), pixel_values is not None, order, owner, True)
            if cands:
                j.try_resume, j.n_candidates = 1, len(cands)
                for i, f in enumerate(cands):
                    j.candidates[i] = f
            apply = self._plan_prefix(j, slot, want) if want is not None else (lambda: self.slot_img.pop(slot, None))
            self.free.remove(slot)
            if has_shape:     # the sequence's length rules and bias pairs (and everything below) go with its join (text or not)
                tp = C.cast(tids.data_ptr(), C.POINTER(C.c_int64)) if tids is not None else None
                rc = self.lib.dtk_engine_submit_shape(self._h, C.byref(j), C.byref(ext), C.c_float(pen_p), C.c_float(pen_f), int(pen_s), C.byref(dry),
                                                      C.byref(lctl), bias_ids, bias_val, len(bias_pairs),
                                                      tp, int(tids.numel()) if tids is not None else 0, C.c_uint64(tkey), C.byref(ticket))
            elif has_dry:     # the sequence's DRY (and its penalties, min_p / epsilon_cutoff) go with its join (text or not)
                tp = C.cast(tids.data_ptr(), C.POINTER(C.c_int64)) if tids is not None else None
                rc = self.lib.dtk_engine_submit_dry(self._h, C.byref(j), C.byref(ext), C.c_float(pen_p), C.c_float(pen_f), int(pen_s), C.byref(dry),
                                                    tp, int(tids.numel()) if tids is not None else 0, C.c_uint64(tkey), C.byref(ticket))
            elif has_pen:     # the sequence's presence / frequency penalty (and its min_p / epsilon_cutoff) go with its join (text or not)
                tp = C.cast(tids.data_ptr(), C.POINTER(C.c_int64)) if tids is not None else None
                rc = self.lib.dtk_engine_submit_pen(self._h, C.byref(j), C.byref(ext), C.c_float(pen_p), C.c_float(pen_f), int(pen_s), tp,
                                                    int(tids.numel()) if tids is not None else 0, C.c_uint64(tkey), C.byref(ticket))
            elif has_ext:     # the sequence's min_p / epsilon_cutoff go with its join (text or not)
                tp = C.cast(tids.data_ptr(), C.POINTER(C.c_int64)) if tids is not None else None
                rc = self.lib.dtk_engine_submit_ext(self._h, C.byref(j), C.byref(ext), tp, int(tids.numel()) if tids is not None else 0,
                                                    C.c_uint64(tkey), C.byref(ticket))
            elif tids is not None:
                rc = self.lib.dtk_engine_submit_text(self._h, C.byref(j), C.cast(tids.data_ptr(), C.POINTER(C.c_int64)), int(tids.numel()),
                                                     C.c_uint64(tkey), C.byref(ticket))
            else:
                rc = self.lib.dtk_engine_submit(self._h, C.byref(j), C.byref(ticket))
            if rc != 0:
                self.free.append(slot)
                raise _lib.DtkError(f"dtk_engine_submit failed ({rc}): {j.error_out.decode(errors='replace')}")
            if cands:
                # owner-less resume candidates: the slot is only known once the join has run, so the bookkeeping waits for it and
                # no other join is planned meanwhile (rare path: MCTS trees always carry an owner)
                held_through = True
                rc = self.lib.dtk_engine_await(self._h, ticket.value)
                if rc == 0 and j.how_out == _lib.DTK_JOIN_RESUMED:
                    if j.slot_out != slot:
                        self.free.append(slot)
                        self.free.remove(j.slot_out)
                        slot = j.slot_out
                elif rc == 0:
                    apply()
            else:
                # (an owner's try_resume join plans a fork from the cache or an in-place reuse — `holds(last)` — and both leave the
                # bookkeeping as it is if the join resumes instead: their `apply` only re-states slot_img[slot] == want)
                apply()
        if not held_through:
            rc = self.lib.dtk_engine_await(self._h, ticket.value)
        joined = rc == 0
        try:
            self._joined(j, joined, f"join of a sequence failed ({rc})")
            yield _NativeSequence(self, slot, logprobs, top)
        finally:
            if joined and self._h:
                self.lib.dtk_engine_leave(self._h, slot)
            with self._cv:
                if not joined:
                    self._forget(slot, j, want)
                self.free.append(slot)
                self._cv.notify_all()
            del ids, px, tids     # (kept alive until here: the native join read them)

    def _check_top(self, top_logprobs, logprobs) -> int:
        """sequence(top_logprobs=j) -> j (0: not asked for); the refusals of an engine built without top_logprobs=, or with a smaller k"""
        if not top_logprobs:
            return 0
        if not self.top_logprobs:
            raise NotImplementedError("top_logprobs: not in the batch engines yet")
        from ..model.modeling import check_top_logprobs
        j = check_top_logprobs(top_logprobs, logprobs)
        if j > self.top_logprobs:
            raise ValueError(f"top_logprobs = {j}: this engine was built with top_logprobs={self.top_logprobs}")
        return j

    def _want_logprobs(self):
        """(under _cv) sequence(logprobs=True): the first such sequence switches the device over, before any sequence holds a slot"""
        if not self._lp:
            if len(self.free) < self.capacity and not self.model.logprobs_enabled:
                raise _lib.DtkError("sequence(logprobs=True): log-probabilities are switched on before the first join, not while "
                                    "sequences hold slots")
            self._enable_logprobs()

    def _joined(self, j, joined: bool, what: str):
        """the outcome of an awaited join: its error, or the engine's counters"""
        if not joined:
            text = j.error_out.decode(errors="replace")
            if "image patch tokens" in text:
                raise ValueError(text[text.index("The "):] if "The " in text else text)      # the reference's own ValueErrors
            raise _lib.DtkError(f"{what}: {text}")
        with self._cv:
            self.joins += 1
            if j.how_out == _lib.DTK_JOIN_RESUMED:
                self.resumes += 1
            elif j.how_out == _lib.DTK_JOIN_IN_PLACE:
                self.inplace_reuses += 1

    def _guided(self, cond, neg, scale, owner, logprobs, tables, pick, top=0):
        """sequence(guidance=...): two slots, two plans (`cond`, `neg`: join, prefix key and tensors of each prompt), one native command
        (dtk_engine_submit_guided) that carries the sequence's `tables`.  The negative branch is planned after the sequence's own
        bookkeeping has been applied, so the two never claim the same prefix-cache slot; an owner's negative branch remembers its slot
        under (owner, "uncond")."""
        ticket = C.c_uint64(0)
        j, gj, tids = cond["j"], neg["j"], cond["tids"]
        g = _lib.DtkGuided()
        g.cond, g.uncond = C.pointer(j), C.pointer(gj)
        g.uncond_text_ids = neg["tids"].data_ptr() if neg["tids"] is not None else None
        g.n_uncond_text = int(neg["tids"].numel()) if neg["tids"] is not None else 0
        g.uncond_text_key, g.scale = neg["tkey"], scale
        slots = []
        with self._cv:
            if logprobs:
                self._want_logprobs()
            while len(self.free) < 2:
                self._cv.wait()
            self._check_adapter_epoch()
            order = sorted(self.free)
            for side, okey in ((cond, owner), (neg, None if owner is None else (owner, "uncond"))):
                slot, _ = pick(side["j"], side["want"], int(side["ids"].numel()), int(side["ids"][-1]), side["has_px"], order, okey, False)
                (self._plan_prefix(side["j"], slot, side["want"]) if side["want"] is not None else (lambda s_=slot: self.slot_img.pop(s_, None)))()
                order = [f for f in order if f != slot]
                slots.append(slot)
            slot, uslot = slots
            self.free.remove(slot)
            self.free.remove(uslot)
            (pen_p, pen_f, pen_s), (bias_ids, bias_val, n_bias) = tables["pen"], tables["bias"]
            tp = C.cast(tids.data_ptr(), C.POINTER(C.c_int64)) if tids is not None else None
            rc = self.lib.dtk_engine_submit_guided(self._h, C.byref(g), C.byref(tables["ext"]), C.c_float(pen_p), C.c_float(pen_f), int(pen_s),
                                                   C.byref(tables["dry"]), C.byref(tables["lctl"]), bias_ids, bias_val, n_bias, tp,
                                                   int(tids.numel()) if tids is not None else 0, C.c_uint64(cond["tkey"]), C.byref(ticket))
            if rc != 0:
                self._forget(slot, j, cond["want"])
                self._forget(uslot, gj, neg["want"])
                self.free += [slot, uslot]
                self._cv.notify_all()
                raise _lib.DtkError(f"dtk_engine_submit_guided failed ({rc}): {j.error_out.decode(errors='replace')}")
        joined = self.lib.dtk_engine_await(self._h, ticket.value) == 0
        try:
            self._joined(j, joined, "join of a guided sequence failed")
            seq = _NativeSequence(self, slot, logprobs, top)
            seq.uncond_slot, seq.how, seq.uncond_how = uslot, int(j.how_out), int(gj.how_out)
            yield seq
        finally:
            if joined and self._h:
                self.lib.dtk_engine_leave(self._h, slot)       # ends both
            with self._cv:
                if not joined:
                    self._forget(slot, j, cond["want"])
                    self._forget(uslot, gj, neg["want"])
                self.free += [slot, uslot]
                self._cv.notify_all()
            del cond, neg     # (the tensors the native join read were kept alive until here)

    def _forget(self, slot, j, want):
        """(under _cv) the prompt did not get into `slot`: it holds nobody's prefix, and neither does the prefix-cache slot the prefix
        was to be encoded into"""
        self.slot_img.pop(slot, None)
        if j.prefix_encode and want is not None and self.prefix_cache.get(want) == j.prefix_src:
            self.prefix_cache.pop(want, None)
