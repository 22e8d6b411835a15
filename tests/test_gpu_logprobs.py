"""Log-probabilities of sampled tokens on the MI355X (dtk_set_option "logprobs"): the LP instantiations of the three samplers against
float64 over given logits, the option-off path, decode against the CPU oracle and against model.score, batched steps of the three
step families (a slot alone == in company, bit for bit), forks, the pipeline, one full-size case."""
from __future__ import annotations

import ctypes as C
import gc
import math
import threading

import numpy as np
import pytest
import torch

from oracle import sampling
from oracle.model import DetikzifyOracle
from oracle.ops import rb
from oracle.synth import tensor_specs
from tests.helpers import ENVELOPE, SLACK_LOGITS, TINY, TINY_CFG, envelope_ratio, rel_l2, sketch_image

pytestmark = pytest.mark.gpu

SAMPLED = dict(do_sample=True, temperature=0.8, top_p=0.95)


@pytest.fixture(scope="module")
def tiny():
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny", synthetic=1234)
    model.enable_logprobs()
    return model, proc


def _weights(model, cfg):
    """every tensor the oracle needs, read back from the device (the rope tables as [T][head_dim / 2], whatever the head dim)"""
    out = {}
    for name, shape, _, _ in tensor_specs(cfg):
        if name.startswith("rope."):
            shape = (cfg["max_positions"], cfg["head_dim"] // 2)
        out[name] = model.read_tensor(name).float().reshape(shape)
    return out


def _oracle_logprobs(oracle, ids, px, first):
    """log-probabilities (float64 log-softmax) of ids[first:] by one oracle: prefill of ids[:first], then one teacher-forced pass"""
    rows = [oracle.prefill(ids[:first], px)]
    if ids.numel() - first > 1:
        rows += list(oracle.extend(ids[first:-1].tolist()))
    logits = torch.stack([r.float() for r in rows])
    return torch.log_softmax(logits.double(), dim=-1).gather(1, ids[first:, None])[:, 0]


def _envelope(tag, dev_lp, lp16, lp32):
    """the project's parity bar (tests/helpers.py), as tests/test_gpu_score.py applies it to log-probabilities"""
    e_dev, e_orc = rel_l2(dev_lp, lp32), rel_l2(lp16, lp32)
    print(f"{tag}: logprob vs fp32 oracle: device {e_dev:.2e}, bf16 oracle {e_orc:.2e}, ratio to the envelope {envelope_ratio(e_dev, e_orc):.2f}")
    assert e_dev <= ENVELOPE * e_orc + SLACK_LOGITS, (tag, e_dev, e_orc)


# ------------------------------------------------------------------------------------------ the samplers over given logits
@pytest.mark.parametrize("mode", ["greedy", "T0.8-p0.95", "T1.3-k50"])
@pytest.mark.parametrize("V", [1000, 1001, 4096, 32000, 40000, 128256])
def test_sampler_op_against_float64(tiny, V, mode):
    """dtk_op_sample_lp: k_sample_fast (V <= 32 768; 1001: the scalar loads of a ragged last thread), the multi-block chain (40 000: its
    first size; 128 256), k_sample (top-k above 32 768).  Token == oracle/sampling.py's; logprob within 2e-5 of float64
    z[t] - logsumexp(z) (an fp32 tree sum of <= 2^17 positive terms is <~ 20 * 2^-24 relative, + 2-ulp expf / logf and one rounding at
    |value| <= 16: <~ 5e-6; the bound is 4 x that); sample_logprob within 1e-6 relative of float64 log(q[t] / total) from the oracle's
    integers (the device forms it in double from the same integers: only the fp32 rounding remains); greedy: exactly 0."""
    model, _ = tiny
    g = torch.Generator().manual_seed(V)
    logits = rb(torch.randn(V, generator=g) * 4)
    order = torch.argsort(logits, descending=True)
    bad, begin = [int(order[0])], [int(order[1])]          # the banned id IS the raw arg-max: logprob is unmasked, the choice is not
    lb = logits.numpy().copy()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ref_lsm = torch.log_softmax(logits.double(), dim=0)
    T, k, p = {"greedy": (1.0, 0, 1.0), "T0.8-p0.95": (0.8, 0, 0.95), "T1.3-k50": (1.3, 50, 1.0)}[mode]
    if mode == "greedy":
        model.set_sampling(do_sample=False, bad_ids=bad, begin_suppress_ids=begin)
    else:
        model.set_sampling(do_sample=True, temperature=T, top_p=p, top_k=k, seed=4711, bad_ids=bad, begin_suppress_ids=begin)
    tok, lp, lp2 = C.c_int64(), (C.c_float * 2)(), (C.c_float * 2)()
    worst_lp = worst_slp = 0.0
    for step in range(8):
        model._check(model.lib.dtk_op_sample_lp(model._ctx, ptr(lb), V, step, C.byref(tok), None, lp), "dtk_op_sample_lp")
        t = tok.value
        if mode == "greedy":
            assert t == sampling.greedy(logits, bad, begin, step == 0)
            assert lp[1] == 0.0 and math.copysign(1.0, lp[1]) == 1.0
        else:
            rt, _ = sampling.draw(logits, T, k, p, 4711, step, bad, begin, step == 0)
            assert t == rt, (step, t, rt)
            z, q = sampling.integer_masses(logits, T, bad, begin, step == 0)
            keep = sampling.kept_mask(z, q, k, p)
            total = int(torch.where(keep, q, torch.zeros_like(q)).sum())
            want = math.log(int(q[t]) / total)
            worst_slp = max(worst_slp, abs(lp[1] - want) / max(abs(want), 1e-30) if want != 0.0 else abs(lp[1]))
        worst_lp = max(worst_lp, abs(lp[0] - float(ref_lsm[t])))
        assert t not in bad and (step or t not in begin)
        model._check(model.lib.dtk_op_sample_lp(model._ctx, ptr(lb), V, step, C.byref(tok), None, lp2), "dtk_op_sample_lp")
        assert tok.value == t and bytes(lp) == bytes(lp2), "a second call gives other bits"
    print(f"op_sample_lp V={V} {mode}: max |d logprob| {worst_lp:.2e}, max rel d sample_logprob {worst_slp:.2e}")
    assert worst_lp <= 2e-5
    assert worst_slp <= 1e-6
    assert float(ref_lsm[bad[0]]) > float(ref_lsm[t])       # the raw arg-max was never chosen, and was more probable than what was


# ------------------------------------------------------------------------------------------ the switch
def test_option_off_is_the_path_without_logprobs():
    """24 greedy + 24 sampled tokens are the same with the option 0 and 1; with 0 the _lp calls fail with DTK_ERR_ARG"""
    from detikzify_amd import _lib
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny", synthetic=1234)
    enc = proc(images=sketch_image(2, 96), return_tensors="pt")
    ids, px = enc.input_ids, enc.pixel_values
    kw = dict(input_ids=ids, pixel_values=px, max_new_tokens=24, eos_token_id=-1, bad_words_ids=[[TINY.image_token_id]], seed=31)
    runs = {}
    for on in (0, 1):
        model.set_option("logprobs", on)
        runs[on] = (model.generate(do_sample=False, **kw), model.generate(**SAMPLED, **kw))
        if not on:
            model.decode_launch()
            tok, lp = C.c_int64(), (C.c_float * 2)()
            assert model.lib.dtk_decode_wait_lp(model._ctx, C.byref(tok), lp) == -1       # DTK_ERR_ARG
            assert b"logprobs" in model.lib.dtk_last_error(model._ctx)
            assert model.decode_wait() >= 0                                             # the step is still there for the plain call
            with pytest.raises(_lib.DtkError, match="logprobs"):
                z8 = np.zeros(8, dtype=np.float32)
                model._check(model.lib.dtk_op_sample_lp(model._ctx, z8.ctypes.data_as(C.c_void_p), 8, 0, C.byref(tok), None, lp), "dtk_op_sample_lp")
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][0].shape[1] == ids.shape[1] + 24
    model._logprobs = True
    out = model.generate(return_logprobs=True, **SAMPLED, **kw)
    assert torch.equal(out.sequences, runs[0][1]) and bool(torch.isfinite(out.logprobs).all())
    with pytest.raises(_lib.DtkError):
        model.set_option("logprobs", 2)


# ------------------------------------------------------------------------------------------ against the oracle, one sequence
@pytest.mark.parametrize("name", ["detikzify-tiny", "detikzify-tiny-tl"])
def test_single_sequence_against_the_oracle_and_model_score(name):
    from detikzify_amd.model import load
    model, proc = load(name, synthetic=1234)
    cfg = model.config.oracle_dict()
    w = _weights(model, cfg)
    enc = proc(images=sketch_image(5, 96), return_tensors="pt")
    ids, px = enc.input_ids[0], enc.pixel_values
    out = model.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=32, eos_token_id=-1,
                         bad_words_ids=[[model.config.image_token_id]], seed=77, return_logprobs=True, **SAMPLED)
    T = ids.numel()
    full = out.sequences[0]
    assert full.numel() == T + 32 and out.logprobs.shape == out.sample_logprobs.shape == (1, 32)
    lp16 = _oracle_logprobs(DetikzifyOracle(cfg, w, precision="bf16"), full, px[0], T)
    lp32 = _oracle_logprobs(DetikzifyOracle(cfg, w, precision="fp32"), full, px[0], T)
    dec = out.logprobs[0].double()
    _envelope(f"{name}: 32 sampled tokens", dec, lp16, lp32)
    assert bool((out.logprobs <= 0).all()) and bool((out.sample_logprobs <= 0).all()) and bool(torch.isfinite(out.sample_logprobs).all())
    # the same positions by model.score (one teacher-forced prefill): the two paths differ by no more than their distances to the fp32
    # oracle added together — both measured here
    sc = model.score(full, px, first=T).logprobs.double()
    d_dec, d_sc = float((dec.sum() - lp32.sum()).abs()), float((sc.sum() - lp32.sum()).abs())
    diff = float((dec.sum() - sc.sum()).abs())
    print(f"{name}: sum logprob decode {float(dec.sum()):.5f}, score {float(sc.sum()):.5f}, fp32 oracle {float(lp32.sum()):.5f}; "
          f"|decode - score| {diff:.2e} <= {d_dec:.2e} + {d_sc:.2e}")
    assert diff <= d_dec + d_sc + 1e-12
    _envelope(f"{name}: model.score of the same tokens", sc, lp16, lp32)


# ------------------------------------------------------------------------------------------ batched steps
def _prompts(proc, n):
    enc = proc(images=sketch_image(7, 96), return_tensors="pt")
    base, px = enc.input_ids[0], enc.pixel_values
    return [torch.cat([base, torch.tensor([20 + 3 * s, 41 + s][: 1 + s % 2], dtype=torch.int64)]) for s in range(n)], px


@pytest.fixture(scope="module", params=[4, 16, 64], ids=lambda n: f"{n}slots")
def batched(request):
    """toy model whose context decodes with the multi-vector family (4), one MFMA column tile (16), four + the prefix kernel (64)"""
    from detikzify_amd.model import load
    n = request.param
    model, proc = load("detikzify-tiny", synthetic=1234, batch_slots=n + 1)
    assert model.max_decode_slots() == n
    model.enable_logprobs()
    yield model, proc, n
    del model
    gc.collect()


def _decode_slots(model, prompts, px, slots, steps, watch):
    for s in slots:
        model.set_sampling(slot=s, seed=900 + s, bad_ids=[TINY.image_token_id], **SAMPLED)
        model.prefill(prompts[s], px, slot=s)
    toks, lps, slps = [], [], []
    for _ in range(steps):
        model.decode_batch_launch(slots)
        t, lp, slp = model.decode_batch_wait_lp()
        assert all(t[s] >= 0 and math.isfinite(lp[s]) for s in slots)
        assert all(t[s] == -1 and math.isnan(lp[s]) and math.isnan(slp[s]) for s in range(64) if s not in slots)
        toks.append([t[s] for s in watch]); lps.append([lp[s] for s in watch]); slps.append([slp[s] for s in watch])
    return torch.tensor(toks), torch.tensor(lps, dtype=torch.float32), torch.tensor(slps, dtype=torch.float32)


def test_a_slot_alone_and_in_company_gives_the_same_bits(batched):
    model, proc, n = batched
    prompts, px = _prompts(proc, n)
    w = n - 1                                         # the watched slot: the last column of the last tile
    alone = _decode_slots(model, prompts, px, [w], 16, [w])
    full = _decode_slots(model, prompts, px, list(range(n)), 16, [w, 0])
    for a, f in zip(alone, full):
        assert torch.equal(a[:, 0], f[:, 0])
    cfg = model.config.oracle_dict()
    wts = _weights(model, cfg)
    for col, s in enumerate((w, 0)):
        ids = torch.cat([prompts[s], full[0][:, col]])
        T = prompts[s].numel()
        lp16 = _oracle_logprobs(DetikzifyOracle(cfg, wts, precision="bf16"), ids, px[0], T)
        lp32 = _oracle_logprobs(DetikzifyOracle(cfg, wts, precision="fp32"), ids, px[0], T)
        _envelope(f"{n} slots, slot {s}", full[1][:, col].double(), lp16, lp32)


@pytest.mark.parametrize("engine", ["native", "python"])
def test_engines_deliver_the_pairs_of_the_sequence_alone(batched, engine):
    from detikzify_amd.infer.batching import BatchEngine
    from detikzify_amd.infer.engine import NativeBatchEngine
    model, proc, n = batched
    prompts, px = _prompts(proc, n)
    k = min(n, 12)
    # (no resume in place: a returning prompt would forward its last token through the decode kernels instead of the prefill GEMMs,
    # other low bits: the comparison below is between two joins of the same kind)
    eng = (NativeBatchEngine if engine == "native" else BatchEngine)(model, max_batch=n, resume_in_place=False)
    got, errs = {}, []

    def run(s, tag):
        try:
            got[(s, tag)] = model.generate(input_ids=prompts[s][None], pixel_values=px, max_new_tokens=16, eos_token_id=-1, seed=500 + s,
                                           bad_words_ids=[[TINY.image_token_id]], return_logprobs=True, **SAMPLED)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    try:
        run(0, "alone")
        ths = [threading.Thread(target=run, args=(s, "batch")) for s in range(k)]
        [t.start() for t in ths]
        [t.join(timeout=120) for t in ths]
        assert not any(t.is_alive() for t in ths) and not errs, errs[:1]
    finally:
        eng.close()
    a, b = got[(0, "alone")], got[(0, "batch")]
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.logprobs, b.logprobs) and torch.equal(a.sample_logprobs, b.sample_logprobs)
    for s in range(k):
        o = got[(s, "batch")]
        assert o.logprobs.shape == (1, 16) and bool(torch.isfinite(o.logprobs).all()) and bool((o.logprobs <= 0).all())


def test_forked_slot_and_full_prefill_give_equal_pairs(batched):
    """a whole-prefix dtk_kv_fork carries bit-identical KV rows and logits: the fork and its source, same seed, decode the same
    tokens and the same pairs (the rule of the fork tests of tests/test_gpu_parity_batched.py)"""
    model, proc, n = batched
    prompts, px = _prompts(proc, n)
    ids = prompts[1]
    for s in (0, 1):
        model.set_sampling(slot=s, seed=123, bad_ids=[TINY.image_token_id], **SAMPLED)
    model.prefill(ids, px, slot=0)
    model.kv_fork(0, 1, ids.numel())
    rows = []
    for _ in range(12):
        model.decode_batch_launch([0, 1])
        t, lp, slp = model.decode_batch_wait_lp()
        rows.append((t[0], t[1], lp[0], lp[1], slp[0], slp[1]))
    for t0, t1, a0, a1, b0, b1 in rows:
        assert t0 == t1 and np.float32(a0).tobytes() == np.float32(a1).tobytes() and np.float32(b0).tobytes() == np.float32(b1).tobytes()


# ------------------------------------------------------------------------------------------ pipeline
def test_pipeline_sample_attaches_one_pair_per_generated_token(tiny):
    from detikzify_amd.infer import DetikzifyPipeline
    model, proc = tiny
    pipe = DetikzifyPipeline(model, proc, metric="fast", temperature=0.8, top_p=0.95, max_length=model.config.num_patches + 40)
    torch.manual_seed(3)
    gen = pipe._generator(sketch_image(1, 96), None, True)
    out = gen.generate(input_ids=gen.montecarlo.root_node.token_ids, return_logprobs=True)
    n_new = out.sequences.shape[1] - gen.montecarlo.root_node.token_ids.numel()
    assert n_new > 0 and out.logprobs.shape == (1, n_new)
    torch.manual_seed(3)
    doc = pipe.sample(sketch_image(1, 96), return_logprobs=True)
    assert len(doc.token_logprobs) == len(doc.token_sample_logprobs) == n_new       # every generated token, EOS included
    assert all(math.isfinite(v) and v <= 0 for v in doc.token_logprobs) and all(math.isfinite(v) and v <= 0 for v in doc.token_sample_logprobs)
    assert doc.token_logprobs == [float(v) for v in out.logprobs[0]]
    assert not hasattr(pipe.sample(sketch_image(1, 96)), "token_logprobs")


# ------------------------------------------------------------------------------------------ full size
def test_full_size_v2_8b_multiblock_chain_in_a_real_step():
    """detikzify-v2-8b (synthetic weights), V = 128 256: the multi-block chain inside the captured step.  8 sampled tokens are the same
    with the option off and on; logprob against float64 log-softmax of the DEVICE's own logits row (dtk_prefill / dtk_get_logits) at
    2e-5 — the bound of the sampler-op test: the row is the same fp32 values the sampler read."""
    from detikzify_amd.model import load
    model, proc = load("detikzify-v2-8b", synthetic=4321, max_positions=512)
    try:
        cfg = model.config
        g = torch.Generator().manual_seed(8)
        ids = torch.randint(3, cfg.vocab - 1, (24,), generator=g)
        ids = ids[ids != cfg.image_token_id]
        samp = dict(seed=99, bad_ids=[cfg.image_token_id], **SAMPLED)
        runs = {}
        for on in (0, 1):
            model.set_option("logprobs", on)
            model.set_sampling(**samp)
            row = model.prefill(ids, None, return_logits=True)
            toks, worst = [], 0.0
            for _ in range(8):
                model.decode_launch()
                if on:
                    t, lp, slp = model.decode_wait_lp()
                    ref = float(torch.log_softmax(row.double(), dim=0)[t])
                    worst = max(worst, abs(lp - ref))
                    assert math.isfinite(slp) and slp <= 0
                    row = model.get_logits()
                else:
                    t = model.decode_wait()
                toks.append(t)
            runs[on] = toks
        print(f"v2-8b: tokens {runs[1]}, max |logprob - log_softmax(device logits)[t]| {worst:.2e}")
        assert runs[0] == runs[1]
        assert worst <= 2e-5
    finally:
        del model
        gc.collect()
