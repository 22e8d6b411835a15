"""Helpers of the guided-engine tests (tests/test_cfg_engine_host.py, tests/test_gpu_cfg_engine.py).

PairDevice    a scripted device without a GPU (DetikzifyForCausalLM above the C-ABI wrappers, as the scripted device of the engine
              tests) that knows guided pairs the way the library does: set_guidance / guidance / reserve_guidance, a step that refuses
              half a pair or a pair in two phases, a conditional token that depends on BOTH contexts and the scale, an unconditional slot
              that follows.  Every device call is logged in `.log`.
pair_steps    steps of a standing pair on a real context, each checked by hand against dtk_op_cfg_mix + the oracle's pick.
"""
import ctypes as C
import threading
import time
import zlib
from types import SimpleNamespace

import numpy as np
import torch

from detikzify_amd.model.modeling import DetikzifyForCausalLM, GenerationConfig

from .helpers import fake_processor, sketch_image

IMG, EOS, VOCAB, NIMG = 1, 2, 512, 12


class _Lib:
    def __init__(self, dev):
        self.dev = dev

    def dtk_context_len_slot(self, ctx, s):
        return len(self.dev.ctx.get(s, ()))

    def dtk_max_decode_slots(self, ctx):       # the rule of include/dtk.h: <= 5 slots -> 0..3 decode; else 16 / 32 / 64 column slots
        n = self.dev.slots
        return min(n, 4 if n <= 5 else (64 if n > 33 else (32 if n > 17 else 16)))


class _Vision:
    def pooled_only(self, pixel_values):
        time.sleep(0.001)
        return torch.nn.functional.adaptive_avg_pool2d(pixel_values.float(), 4).flatten() + 1.5

    def __call__(self, pixel_values, **_):
        return SimpleNamespace(pooler_output=self.pooled_only(pixel_values)[None], last_hidden_state=None)


class PairDevice(DetikzifyForCausalLM):
    SINGLE = -1

    def __init__(self, slots=0, max_positions=160):      # no super().__init__: that one creates the device context
        cfg = SimpleNamespace(image_token_id=IMG, eos_token_id=EOS, pad_token_id=0, bos_token_id=1, vocab=VOCAB,
                              max_positions=max_positions, pooling_mode="cos")
        cfg.text_config = cfg
        self.config = cfg
        self.generation_config = GenerationConfig(eos_token_id=EOS, pad_token_id=0, bos_token_id=1)
        self.name_or_path = "scripted"
        self.model = SimpleNamespace(vision_model=_Vision())
        self.reuse_prefix, self.batch_engine, self._weights_ready = False, None, True
        self._vit_lock, self._single_busy = threading.RLock(), threading.Lock()
        self.lib, self._ctx, self.slots = _Lib(self), None, slots
        self.ctx, self.img, self.samp, self.gen0 = {}, {}, {}, {}
        self.pending, self.bpending = [], []
        self.prefills = self.forks = self.tail_prefills = self.resumes = 0
        self.forced = {}
        self.pairs = {}             # cond slot -> (uncond slot, scale)
        self.reserved = 0
        self.log = []               # (name, *args) of every device call, in order
        self.fail_prefill_of = None         # a prompt length whose prefill raises (a scripted failure)
        self.disagree_at = None             # (cond slot, context length): the unconditional slot reports another token there
        tok = fake_processor(VOCAB, NIMG).tokenizer
        self.newline = [i for i, t in enumerate(tok._id2tok) if "\n" in t and i > 2]
        self.plain = [i for i, t in enumerate(tok._id2tok) if "\n" not in t and i > 2]

    # ---- the toy LM: the next token is a hash of what the slot (a pair: both slots and the scale) holds -------------------------
    def _pick(self, s, state):
        sp = self.samp[s]
        seed = sp.get("seed", 0) if sp.get("do_sample") else 0
        h = zlib.crc32(repr((state, seed)).encode())
        r, pick = (h & 0xFFFF) / 65536.0, h >> 16
        first = len(self.ctx[s]) == self.gen0[s]
        if r < 0.05 and not (first and EOS in sp.get("begin_suppress_ids", ())) and EOS not in sp.get("always_suppress_ids", ()):
            return EOS
        return self.newline[pick % len(self.newline)] if r < 0.4 else self.plain[pick % len(self.plain)]

    def _step(self, slots):
        out = {}
        followers = {u: c for c, (u, _) in self.pairs.items()}
        for c, (u, _) in self.pairs.items():
            assert (c in slots) == (u in slots), f"half of the pair ({c}, {u}) in a step"
            if c in slots:
                assert (c in self.forced) == (u in self.forced), f"the pair ({c}, {u}) is in two phases"
        for s in slots:
            if s in followers:
                continue
            if s in self.forced:
                out[s] = self.forced.pop(s)
            elif s in self.pairs:
                u, g = self.pairs[s]
                out[s] = self._pick(s, (self.img[s], self.ctx[s], self.img[u], self.ctx[u], g))
            else:
                out[s] = self._pick(s, (self.img[s], self.ctx[s]))
        for u, c in followers.items():
            if u in slots:
                out[u] = self.forced.pop(u) if u in self.forced else out[c]
                if self.disagree_at == (c, len(self.ctx[c])):
                    out[u] = out[c] + 1
        for s in slots:
            self.ctx[s] = self.ctx[s] + [out[s]]
        return out

    # ---- C-ABI wrappers of modeling.py, scripted -----------------------------------------------------------------------------
    def num_slots(self):
        return self.slots

    def set_sampling(self, do_sample=False, temperature=1.0, top_p=1.0, top_k=0, seed=0, bad_ids=(), begin_suppress_ids=(),
                     always_suppress_ids=(), slot=None):
        self.log.append(("set_sampling", slot, bool(do_sample)))
        self.samp[self.SINGLE if slot is None else slot] = dict(
            do_sample=do_sample, seed=seed, bad_ids=tuple(bad_ids), begin_suppress_ids=tuple(begin_suppress_ids),
            always_suppress_ids=tuple(always_suppress_ids))

    def prefill(self, input_ids, pixel_values=None, return_logits=False, reuse=None, slot=None):
        assert not self.bpending, "prefill while a batched step is un-collected"
        s = self.SINGLE if slot is None else slot
        ids = [int(t) for t in input_ids.reshape(-1)]
        self.log.append(("prefill", s, len(ids)))
        if self.fail_prefill_of == len(ids):
            raise RuntimeError("scripted prefill failure")
        key = self.image_key(pixel_values) if pixel_values is not None else 0
        if reuse:
            n = next((i for i, t in enumerate(ids) if t != IMG), len(ids))
            assert self.img.get(s) == key and self.ctx[s][:n] == ids[:n], "prefix reuse without the prefix in the slot"
            self.tail_prefills += 1
        self.pending.clear()
        self.ctx[s], self.img[s], self.gen0[s] = ids, key, len(ids)
        self.forced.pop(s, None)
        self.prefills += 1

    def kv_fork(self, src_slot, dst_slot, n_tokens):
        self.log.append(("kv_fork", src_slot, dst_slot, n_tokens))
        assert len(self.ctx[src_slot]) >= n_tokens
        self.ctx[dst_slot], self.img[dst_slot] = self.ctx[src_slot][:n_tokens], self.img[src_slot]
        self.gen0[dst_slot] = n_tokens
        self.forced.pop(dst_slot, None)
        self.forks += 1

    def best_lcp_slot(self, slots, ids, key=0):
        ids, best = [int(t) for t in ids.reshape(-1)], None
        for s in slots:
            if s not in self.ctx or self.img.get(s) != key:
                continue
            n = next((i for i, (a, b) in enumerate(zip(self.ctx[s], ids)) if a != b), min(len(self.ctx[s]), len(ids)))
            if n > (best[1] if best else 0):
                best = (s, n)
        return best

    def resume_slot(self, slot, ids, key=0):
        ids = [int(t) for t in ids.reshape(-1)]
        self.log.append(("resume", slot, len(ids)))
        assert self.img.get(slot) == key and self.ctx[slot][:len(ids) - 1] == ids[:-1], "resume without the prompt in the slot"
        assert not any(slot in step for step in self.bpending), "resume of a slot that is part of an un-collected step"
        self.ctx[slot], self.gen0[slot], self.forced[slot] = ids[:-1], len(ids), ids[-1]
        self.resumes += 1

    def decode_launch(self):
        assert len(self.ctx[self.SINGLE]) < self.config.max_positions
        self.pending.append(self._step([self.SINGLE])[self.SINGLE])

    def decode_wait(self):
        return self.pending.pop(0)

    def decode_batch_launch(self, active_slots):
        slots = list(active_slots)
        self.log.append(("launch", tuple(slots)))
        assert len(self.bpending) < 2 and slots == sorted(slots)
        self.bpending.append(self._step(slots))

    def decode_batch_wait(self):
        time.sleep(0.0002)
        step = self.bpending.pop(0)
        return [step.get(s, -1) for s in range(64)]

    def synchronize(self):
        pass

    # ---- pairs, as the library keeps them ------------------------------------------------------------------------------------------
    def set_guidance(self, scale, cond_slot, uncond_slot):
        assert not self.bpending, "the pair table is written with a step in flight"
        g = 1.0 if scale is None else float(scale)
        self.log.append(("set_guidance", cond_slot, uncond_slot, g))
        if uncond_slot is None or uncond_slot < 0 or g == 1.0:
            self.pairs.pop(cond_slot, None)
            return
        taken = {s for c, (u, _) in self.pairs.items() if c != cond_slot for s in (c, u)}
        assert cond_slot != uncond_slot and cond_slot not in taken and uncond_slot not in taken, "slot already in another pair"
        self.pairs[cond_slot] = (uncond_slot, g)

    def guidance(self, slot):
        for c, (u, g) in self.pairs.items():
            if slot in (c, u):
                return dict(partner=u if slot == c else c, is_cond=slot == c, scale=g, lse=(0.0, 0.0))
        return None

    def reserve_guidance(self, n_pairs):
        self.log.append(("reserve_guidance", int(n_pairs)))
        self.reserved = int(n_pairs)


def prompt(proc, image_seed, extra=()):
    enc = proc(images=sketch_image(image_seed, 96), return_tensors="pt")
    ids = torch.cat([enc.input_ids[0], torch.tensor(list(extra), dtype=torch.int64)])
    return ids, enc.pixel_values


def threads(n, target):
    errs = []

    def guarded(k):
        try:
            target(k)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    ths = [threading.Thread(target=guarded, args=(k,)) for k in range(n)]
    [t.start() for t in ths]
    [t.join(timeout=90) for t in ths]
    assert not any(t.is_alive() for t in ths), "threads hang"
    assert not errs, errs[:1]


# ---- a real context ------------------------------------------------------------------------------------------------------------------
def op_cfg_mix(model, zc, zu, g):
    """dtk_op_cfg_mix: (out float32 [V], (Lc, Lu) float32)"""
    zc, zu = np.ascontiguousarray(zc, np.float32), np.ascontiguousarray(zu, np.float32)
    out, lse = np.empty(zc.size, np.float32), (C.c_float * 2)()
    rc = model.lib.dtk_op_cfg_mix(model._ctx, zc.ctypes.data_as(C.c_void_p), zu.ctypes.data_as(C.c_void_p), zc.size, float(g),
                                  out.ctypes.data_as(C.c_void_p), lse)
    model._check(rc, "dtk_op_cfg_mix")
    return out, (float(lse[0]), float(lse[1]))


def bits(values):
    return np.asarray(values, np.float32).tobytes()


def pick(row, cfg, n, cur, bad, **shape):
    """the oracle's token over the (mixed) row: draw index n, sequence length cur"""
    from oracle import sampling
    from tests import shape_oracle
    row = torch.from_numpy(np.asarray(row, dtype=np.float32).copy())
    if shape:
        if cfg["do_sample"]:
            return shape_oracle.draw(row, cur, cfg["temperature"], cfg["top_k"], cfg["top_p"], cfg["seed"], n, bad=bad, **shape)[0]
        return shape_oracle.greedy(row, cur, bad=bad, **shape)
    if cfg["do_sample"]:
        return sampling.draw(row, cfg["temperature"], cfg["top_k"], cfg["top_p"], cfg["seed"], n, bad=bad)[0]
    return sampling.greedy(row, bad=bad)


LSE_TOL = 2e-5


def pair_steps(model, c, u, cfg, g, steps, cur, bad, company=None, counted=None, pp=0.0, pairs=None, n0=0):
    """`steps` steps of the standing pair (c, u), each checked by hand: before the launch both pending rows are read back and mixed by
    dtk_op_cfg_mix (the same kernels, hence the same bits as the step's); both slots' tokens must be the oracle's pick over that row,
    the log-probability the float64 log-softmax of that row at the token, dtk_get_guidance's (Lc, Lu) the op's.  Returns (tokens,
    logprob bytes, the company slot's tokens)"""
    from tests import cfg_oracle
    toks, lpb, beside = [], [], []
    counted = list(counted or [])
    shape = dict(pairs=pairs, pp=pp) if (pp or pairs) else {}
    active = sorted([c, u] + ([company] if company is not None else []))
    for n in range(steps):
        zc, zu = model.get_logits_slot(c).numpy(), model.get_logits_slot(u).numpy()
        mixed, lse = op_cfg_mix(model, zc, zu, g)
        model.decode_batch_launch(active)
        t, lp, slp = model.decode_batch_wait_lp()
        want = pick(mixed, cfg, n0 + n, cur + n, bad, **({**shape, "counted": counted + toks} if shape else {}))
        assert t[c] == want and t[u] == want, (n, t[c], t[u], want)
        ref = cfg_oracle.logprob64(mixed, want)
        assert abs(lp[c] - ref) <= LSE_TOL, (n, lp[c], ref)
        assert bits([lp[u], slp[u]]) == bits([lp[c], slp[c]])          # the follower copied the ring entries
        got = model.guidance(c)["lse"]
        assert bits(got) == bits(lse), (n, got, lse)
        toks.append(int(want))
        lpb.append(bits([lp[c], slp[c]]))
        if company is not None:
            beside.append(int(t[company]))
    return toks, lpb, beside
