"""min_p / epsilon_cutoff without a GPU: the integer restatement (tests/trunc_oracle.py) against the installed transformers' warpers,
hand cases with exact integers, the additive C ABI, generate()'s argument gate, and the ext call of both batch engines over the
scripted device."""
from __future__ import annotations

import ctypes as C
import re
import threading
from pathlib import Path

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from detikzify_amd.infer.batching import BatchEngine
from detikzify_amd.infer.engine import NativeBatchEngine
from oracle import sampling

from . import trunc_oracle
from .helpers import fake_processor
from .test_generate_loop import EOS, IMG, NIMG, VOCAB, ScriptedDevice, _prompt

ONE = 1 << 31
HEADER = (Path(__file__).resolve().parents[1] / "include" / "dtk.h").read_text()


# ------------------------------------------------------------------------------------------ against HF's warpers
def _hf_kept(logits, T, top_k, top_p, min_p, eps):
    from transformers.generation.logits_process import (EpsilonLogitsWarper, MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    s = logits[None].clone()
    chain = [TemperatureLogitsWarper(T)] if T != 1.0 else []
    if top_k:
        chain.append(TopKLogitsWarper(top_k))
    if top_p < 1.0:
        chain.append(TopPLogitsWarper(top_p))
    chain.append(MinPLogitsWarper(min_p))
    if eps > 0:
        chain.append(EpsilonLogitsWarper(eps))
    for w in chain:
        s = w(None, s)
    return torch.isfinite(s[0])


def _near_a_boundary(logits, T, top_k, top_p, min_p, eps, rel=1e-5):
    """a row on which fp32 softmax arithmetic (HF) and integer masses may legitimately disagree: some exp(z - zmax) within `rel` of
    min_p, or a kept token's probability within `rel` of eps or of the top-p boundary (float64 restatement of HF's chain)"""
    z = (logits.double() / T)
    ratio = torch.exp(z - z.max())
    if bool(((ratio - min_p).abs() <= rel * min_p).any()):
        return True
    keep = torch.ones_like(z, dtype=torch.bool)
    if top_k:
        keep &= z >= torch.topk(z, top_k)[0][-1]
    if top_p < 1.0:
        p = torch.where(keep, ratio, torch.zeros_like(ratio))
        p = p / p.sum()
        srt, idx = torch.sort(p)                      # ascending, as HF: remove cumsum <= 1 - top_p
        cum = srt.cumsum(0)
        live = srt > 0
        if bool((((cum - (1 - top_p)).abs() <= rel) & live).any()):
            return True
        rm = cum <= (1 - top_p)
        rm[-1] = False
        keep &= ~torch.zeros_like(rm).scatter(0, idx, rm)
    keep &= ratio >= min_p
    if eps > 0:
        p = torch.where(keep, ratio, torch.zeros_like(ratio))
        p = p / p.sum()
        if bool((((p - eps).abs() <= rel * eps) & keep).any()):
            return True
    return False


def test_kept_set_is_hf_min_p_and_epsilon_behind_top_k_top_p():
    g = torch.Generator().manual_seed(20240611)
    rows = skipped = 0
    temps, min_ps, epss = (0.7, 1.0, 1.3), (0.02, 0.1, 0.5), (0.0, 3e-4, 3e-3)
    for r in range(200):
        logits = torch.randn(1000, generator=g) * 3
        T, min_p, eps = temps[r % 3], min_ps[(r // 3) % 3], epss[(r // 9) % 3]
        top_k, top_p = ((50, 0.9) if (r // 27) % 2 else (0, 1.0))
        rows += 1
        if _near_a_boundary(logits, T, top_k, top_p, min_p, eps):
            skipped += 1
            continue
        _, _, keep = trunc_oracle.kept_set(logits, T, top_k, top_p, min_p, eps)
        hf = _hf_kept(logits, T, top_k, top_p, min_p, eps)
        assert torch.equal(keep, hf), (r, T, top_k, top_p, min_p, eps, int(keep.sum()), int(hf.sum()))
    print(f"HF restatement: {rows} rows, {skipped} skipped near a boundary")
    assert rows == 200 and skipped <= rows // 10


# ------------------------------------------------------------------------------------------ exact integers
def test_hand_cases_with_exact_integers():
    # all equal: every mass is 2^31, min_p = 1 keeps all, any eps < 1 / V keeps all, eps above 1 / V leaves the lowest id
    flat = torch.zeros(8)
    z, q, keep = trunc_oracle.kept_set(flat, 1.0, 0, 1.0, min_p=1.0)
    assert q.tolist() == [ONE] * 8 and bool(keep.all())
    _, _, keep = trunc_oracle.kept_set(flat, 1.0, 0, 1.0, eps=0.1)            # qe = int(f32(0.1) * 8 * 2^31) <= 2^31
    assert int(np.float64(np.float32(0.1)) * np.float64(8 * ONE)) < ONE and bool(keep.all())
    _, _, keep = trunc_oracle.kept_set(flat, 1.0, 0, 1.0, eps=0.2)            # qe > 2^31: nothing passes, the fallback
    assert keep.tolist() == [True] + [False] * 7
    tok, probs, slp = trunc_oracle.draw(flat, 1.0, 0, 1.0, seed=3, n=5, eps=0.2)
    assert tok == 0 and probs.tolist() == [1.0] + [0.0] * 7 and slp == 0.0

    # two-way tie at the maximum, min_p = 1: exactly the entries with q = 2^31
    row = torch.tensor([0.5, 2.0, -1.0, 2.0, 1.999])
    z, q, keep = trunc_oracle.kept_set(row, 1.0, 0, 1.0, min_p=1.0)
    assert keep.tolist() == [False, True, False, True, False] and int(q[1]) == int(q[3]) == ONE and int(q[4]) < ONE
    assert trunc_oracle.qmin_of(1.0) == ONE and trunc_oracle.qmin_of(0.5) == ONE // 2
    toks = {trunc_oracle.draw(row, 1.0, 0, 1.0, seed=11, n=n, min_p=1.0)[0] for n in range(64)}
    assert toks == {1, 3}

    # eps removes everything; the tie at the maximum falls to the lowest id, also behind top-k / top-p / min-p
    row = torch.tensor([1.0, 3.0, 3.0, 2.9, 2.8, 0.0])
    _, _, keep = trunc_oracle.kept_set(row, 1.0, 0, 1.0, eps=0.6)
    assert keep.tolist() == [False, True, False, False, False, False]
    _, _, keep = trunc_oracle.kept_set(row, 1.0, 4, 0.99, min_p=0.5, eps=0.6)
    assert keep.tolist() == [False, True, False, False, False, False]
    # ... and an eps that keeps the two maxima but not the rest: q >= qe exactly
    z, q, k0 = trunc_oracle.kept_set(row, 1.0, 0, 1.0)
    qe = int(np.float64(np.float32(0.25)) * np.float64(int(q.sum())))
    _, _, keep = trunc_oracle.kept_set(row, 1.0, 0, 1.0, eps=0.25)
    assert keep.tolist() == (q >= qe).tolist() and keep.tolist()[1:3] == [True, True]

    # off is oracle.sampling.draw, bit for bit
    g = torch.Generator().manual_seed(9)
    for T, k, p in ((0.8, 0, 0.95), (1.2, 50, 0.9), (1.0, 0, 1.0)):
        logits = torch.randn(1000, generator=g) * 3
        for n in range(8):
            t0, p0 = sampling.draw(logits, T, k, p, 77, n, [1], [2], n == 0)
            t1, p1, _ = trunc_oracle.draw(logits, T, k, p, 77, n, 0.0, 0.0, [1], [2], n == 0)
            assert t0 == t1 and torch.equal(p0, p1)


# ------------------------------------------------------------------------------------------ the C ABI
NEW = {
    "dtk_set_sampling_ext": "(dtk_ctx* ctx, const dtk_sampling_ext* x)",
    "dtk_set_sampling_slot_ext": "(dtk_ctx* ctx, int slot, const dtk_sampling_ext* x)",
    "dtk_op_sample_ext": "(dtk_ctx* ctx, const float* logits, int V, int step, int64_t* token_out, float* filtered_probs_out, "
                         "float* lp_out /* [2] or NULL */, const dtk_sampling_ext* x)",
    "dtk_engine_submit_ext": "(dtk_engine* e, dtk_join* j, const dtk_sampling_ext* x, const int64_t* text_ids, int n_text, uint64_t text_key, "
                             "uint64_t* ticket_out)",
    "dtk_engine_set_sampling_ext_op": "(dtk_engine* e, int (*set_sampling_slot_ext)(void* dev, int slot, const dtk_sampling_ext* x))",
}


def test_abi_is_additive_and_bound():
    assert _lib.DTK_ABI_VERSION == 7 and re.search(r"#define DTK_ABI_VERSION 7\b", HEADER)
    flat = re.sub(r"\s+", " ", HEADER)
    X, F, I64, U64 = C.POINTER(_lib.DtkSamplingExt), C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    P = C.c_void_p
    bound = {       # the header's parameter lists above, as ctypes (pointers to anything else: void*)
        "dtk_set_sampling_ext": [P, X],
        "dtk_set_sampling_slot_ext": [P, C.c_int, X],
        "dtk_op_sample_ext": [P, P, C.c_int, C.c_int, I64, P, F, X],
        "dtk_engine_submit_ext": [P, C.POINTER(_lib.DtkJoin), X, I64, C.c_int, C.c_uint64, U64],
        "dtk_engine_set_sampling_ext_op": [P, _lib.DtkEngineOps.SAMPLING_EXT],
    }
    for name, params in NEW.items():
        assert f"int {name}{params};" in flat.replace("int  ", "int "), name
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and list(args) == bound[name], name
    # dtk_op_sample_ext is dtk_op_sample_lp's signature plus the struct
    assert list(_lib.SYMBOLS["dtk_op_sample_ext"][1][:-1]) == list(_lib.SYMBOLS["dtk_op_sample_lp"][1])
    assert _lib.DtkEngineOps.SAMPLING_EXT._argtypes_ == (C.c_void_p, C.c_int, C.POINTER(_lib.DtkSamplingExt))
    # the struct: two floats and six reserved words, as the header spells it
    m = re.search(r"typedef struct dtk_sampling_ext \{(.*?)\} dtk_sampling_ext;", HEADER, re.S)
    fields = re.findall(r"^\s*(float|int32_t)\s+(\w+)(?:\[(\d+)\])?;", m.group(1), re.M)
    assert fields == [("float", "min_p", ""), ("float", "epsilon_cutoff", ""), ("int32_t", "reserved", "6")]
    assert [f[0] for f in _lib.DtkSamplingExt._fields_] == ["min_p", "epsilon_cutoff", "reserved"] and C.sizeof(_lib.DtkSamplingExt) == 32
    lib = _lib.load_library()
    assert lib.dtk_abi_version() == 7
    assert lib.dtk_abi_struct_size(12) == C.sizeof(_lib.DtkSamplingExt) == 32
    # the pinned layouts did not move
    assert lib.dtk_abi_struct_size(1) == C.sizeof(_lib.DtkSampling) == 136
    assert lib.dtk_abi_struct_size(10) == _lib.DtkJoin.error_out.offset
    assert lib.dtk_abi_struct_size(9) == _lib.DtkJoin.sampling.offset and lib.dtk_abi_struct_size(6) == C.sizeof(_lib.DtkJoin)
    assert lib.dtk_abi_struct_size(13) == -1
    # null / misuse is an error code, not a crash
    x = _lib.DtkSamplingExt(min_p=0.1)
    assert lib.dtk_set_sampling_ext(None, C.byref(x)) == -1 and lib.dtk_set_sampling_slot_ext(None, 0, C.byref(x)) == -1
    assert lib.dtk_engine_set_sampling_ext_op(None, _lib.DtkEngineOps.SAMPLING_EXT()) == -1


# ------------------------------------------------------------------------------------------ generate()'s gate
class ExtDevice(ScriptedDevice):
    """the scripted device + a record of every sampling call: ("plain", slot) and ("ext", slot, min_p, epsilon_cutoff)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def set_sampling(self, *a, slot=None, **kw):
        self.calls.append(("plain", slot))
        super().set_sampling(*a, slot=slot, **kw)

    def set_sampling_ext(self, min_p=0.0, epsilon_cutoff=0.0, slot=None):
        self.calls.append(("ext", slot, round(float(min_p), 6), round(float(epsilon_cutoff), 6)))


def test_generate_takes_min_p_and_epsilon_cutoff_and_still_refuses_the_rest():
    dev, proc = ExtDevice(), fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0)
    kw = dict(input_ids=ids[None], pixel_values=px, bad_words_ids=[[IMG]], max_new_tokens=4, do_sample=True, seed=5)
    plain = dev.generate(**kw)
    assert dev.calls == [("plain", None)]
    dev.calls.clear()
    assert torch.equal(dev.generate(min_p=0.1, **kw), plain)              # (the toy LM ignores the sampler's parameters)
    assert dev.calls == [("plain", None), ("ext", None, 0.1, 0.0)]
    dev.calls.clear()
    dev.generate(epsilon_cutoff=3e-4, **kw)
    assert dev.calls == [("plain", None), ("ext", None, 0.0, 3e-4)]
    dev.calls.clear()
    dev.generate(min_p=0.0, epsilon_cutoff=0.0, **kw)                     # HF's neutral values: nothing to set
    dev.generate(min_p=None, epsilon_cutoff=None, **kw)
    assert dev.calls == [("plain", None)] * 2
    dev.generation_config.min_p = 0.25                                    # a checkpoint's generation_config.json is honoured
    dev.calls.clear()
    dev.generate(**kw)
    assert dev.calls == [("plain", None), ("ext", None, 0.25, 0.0)]
    del dev.generation_config.min_p
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=re.escape("`min_p` has to be a float in the [0, 1] interval")):
            dev.generate(min_p=bad, **kw)
    for bad in (-1e-3, 1.0, 2.0, float("nan")):
        with pytest.raises(ValueError, match=re.escape("`epsilon_cutoff` has to be a float > 0 and < 1")):
            dev.generate(epsilon_cutoff=bad, **kw)
    with pytest.raises(NotImplementedError):
        dev.generate(typical_p=0.9, **kw)
    with pytest.raises(NotImplementedError):
        dev.generate(eta_cutoff=1e-3, **kw)
    assert dev.generate(typical_p=1.0, eta_cutoff=0.0, **kw).shape == plain.shape
    # the plain scripted device (no such call on its "library") still decodes, and says so when asked for a value
    old = ScriptedDevice()
    assert torch.equal(old.generate(**kw), plain)
    with pytest.raises(_lib.DtkError, match="min_p"):
        old.generate(min_p=0.1, **kw)


# ------------------------------------------------------------------------------------------ both engines
@pytest.mark.parametrize("engine", [NativeBatchEngine, BatchEngine], ids=["native", "python"])
def test_engines_apply_the_ext_values_behind_the_plain_call_and_reset_them(engine):
    proc = fake_processor(VOCAB, NIMG)
    dev = ExtDevice(slots=5)
    eng = engine(dev, max_batch=1, share_prefix=False)           # one decoding slot: both sequences take slot 0
    try:
        ids, px = _prompt(proc, 1)
        kw = dict(input_ids=ids[None], pixel_values=px, bad_words_ids=[[IMG]], max_new_tokens=5, do_sample=True, eos_token_id=-1)
        a = dev.generate(seed=1, min_p=0.1, epsilon_cutoff=3e-4, **kw)
        b = dev.generate(seed=2, **kw)
    finally:
        eng.close()
    assert a.shape[1] == b.shape[1] == ids.numel() + 5
    assert dev.calls == [("plain", 0), ("ext", 0, 0.1, 3e-4), ("plain", 0), ("ext", 0, 0.0, 0.0)]
    # out of range never reaches the device
    dev2 = ExtDevice(slots=5)
    eng = engine(dev2, max_batch=1, share_prefix=False)
    try:
        with pytest.raises(ValueError, match="min_p"):
            with eng.sequence(ids, px, dict(do_sample=True, min_p=1.5)):
                pass
    finally:
        eng.close()


def test_native_engine_without_the_op_refuses_a_join_with_values():
    """an engine of dtk_engine_create_ops that was given no ext op: a join with values fails in submit, one with 0 / 0 joins"""
    proc = fake_processor(VOCAB, NIMG)
    dev = ScriptedDevice(slots=5)
    eng = NativeBatchEngine(dev, max_batch=2, share_prefix=False)
    lib = _lib.load_library()
    try:
        assert lib.dtk_engine_set_sampling_ext_op(eng._h, _lib.DtkEngineOps.SAMPLING_EXT()) == 0       # take the op away again
        ids, px = _prompt(proc, 2)
        with pytest.raises(_lib.DtkError, match="dtk_engine_set_sampling_ext_op"):
            with eng.sequence(ids, px, dict(do_sample=True, seed=3, min_p=0.2), max_new_tokens=3):
                pass
        out = dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=3, do_sample=True, seed=3, eos_token_id=-1)
        assert out.shape[1] == ids.numel() + 3
        j, t = _lib.DtkJoin(), C.c_uint64()
        bad = _lib.DtkSamplingExt(min_p=2.0)
        assert lib.dtk_engine_submit_ext(eng._h, C.byref(j), C.byref(bad), None, 0, 0, C.byref(t)) == -1 and b"min_p" in j.error_out
        assert lib.dtk_engine_submit_ext(eng._h, C.byref(j), None, None, 0, 0, C.byref(t)) == -1
    finally:
        eng.close()
