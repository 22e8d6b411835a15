"""min_p / epsilon_cutoff on the MI355X: the TR instantiations of the three sampler families over given logits (dtk_op_sample_ext) against
tests/trunc_oracle.py, the off path against dtk_op_sample_lp, one sequence end to end over the device's own logits, and batched steps
of the multi-vector and the MFMA family, driven from the host and by both engines."""
from __future__ import annotations

import ctypes as C
import gc
import math
import threading

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from oracle import sampling
from oracle.ops import rb
from tests import trunc_oracle
from tests.helpers import TINY, sketch_image

pytestmark = pytest.mark.gpu

# One V per sampler family, by the launchers' own rule (csrc/kernels_decode.hip launch_sample_b, csrc/dtk_ops.hip op_sample_impl):
#   "if (sample_mb_preferred(V, do_sample) && !needs_topk) launch_sample_mb(...); else launch_sample(...)"  with
#   sample_mb_supported(V) = V > 32768,  needs_topk = do_sample && 0 < top_k < V,  and inside launch_sample:
#   "sample_fast_ok(a) = a.V <= SF_PER * SAMPLE_THREADS" (= 32 768) -> k_sample_fast, else k_sample.
# So 32 000 is k_sample_fast whatever top_k is; 32 769 is the smallest V that reaches k_sample, and only with 0 < top_k < V (its rows
# that want "no top-k" ask for V - 1); 40 000 is the chain without top-k and k_sample with it.
FAMILIES = {32000: "k_sample_fast", 32769: "k_sample", 40000: "k_smb_*"}
BAD, BEGIN, SEED = [1], [2], 4711


def _bigvocab(slots=0):
    """tiny-v2 with a 40 000-token vocabulary (the recipe of tests/test_gpu_topk.py's fixture)"""
    from detikzify_amd.model.config import preset
    from detikzify_amd.model.modeling import DetikzifyForCausalLM
    cfg = preset("detikzify-tiny-v2")
    cfg.vocab, cfg.name_or_path, cfg.batch_slots = 40000, "detikzify-tiny-v2-bigvocab", slots
    m = DetikzifyForCausalLM(cfg, 0)
    m.fill_synthetic(99)
    return m


@pytest.fixture(scope="module")
def big():
    m = _bigvocab()
    m.enable_logprobs()
    yield m
    del m
    gc.collect()


def _rows(V):
    """8 rows of (tag, logits, T, top_k, top_p, min_p, eps); at 32 769 every row carries a top-k (see FAMILIES)"""
    g = torch.Generator().manual_seed(V)
    nk = V - 1 if V == 32769 else 0
    wide = lambda: rb(torch.randn(V, generator=g) * 4)
    flat = rb(torch.randn(V, generator=g))                  # p_max ~ 1e-3 < 0.05: the epsilon of row 4 leaves nothing
    peaked = wide().clone(); peaked[V // 3] = peaked.max() + 30.0
    tie = wide().clone(); tie[[V - 5, 17]] = tie.max() + 1.0
    return [("min_p .05", wide(), 1.0, nk, 1.0, 0.05, 0.0),
            ("min_p .5", wide(), 1.2, nk, 1.0, 0.5, 0.0),
            ("min_p 1", wide(), 0.8, nk, 1.0, 1.0, 0.0),
            ("eps 3e-4", wide(), 1.0, nk, 1.0, 0.0, 3e-4),
            ("eps .05 fallback", flat, 1.0, nk, 1.0, 0.0, 0.05),
            ("both + k50 + p.9", wide(), 1.2, 50, 0.9, 0.1, 3e-4),
            ("peaked", peaked, 1.0, nk, 0.95, 0.1, 3e-4),
            ("tie at the max", tie, 1.0, nk, 1.0, 0.5, 1e-3)]


def _oracle_row(logits, T, k, p, min_p, eps, first):
    """(z, q, kept masses, kept_total) of one row: the kept set is the same for every draw counter with the same `first`"""
    z, q, keep = trunc_oracle.kept_set(logits, T, k, p, min_p, eps, BAD, BEGIN, first)
    qk = torch.where(keep, q, torch.zeros_like(q))
    return qk, int(qk.sum()), torch.cumsum(qk, 0)


def _oracle_token(run, total, n):
    target = (total * sampling.rand32(SEED, n)) >> 32
    return int(torch.searchsorted(run, torch.tensor(target, dtype=torch.int64), right=True))


@pytest.mark.parametrize("V", list(FAMILIES), ids=[f"{v}-{k}" for v, k in FAMILIES.items()])
def test_op_sample_ext_matches_the_oracle(big, V):
    """token and filtered probabilities exact (the comparison of tests/test_gpu_parity.py::test_op_sample_matches_oracle: equal kept
    sets, probabilities to 1e-5 relative — both sides divide the same two integers); sample_logprob to 1e-6 relative (formed in double
    from the same integers: only the fp32 rounding remains); logprob the bits dtk_op_sample_lp gives for the same token"""
    model = big
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    tok, tok2, lp, lp2 = C.c_int64(), C.c_int64(), (C.c_float * 2)(), (C.c_float * 2)()
    probs = np.empty(V, dtype=np.float32)
    same_tok = fell_back = 0
    for tag, logits, T, k, p, min_p, eps in _rows(V):
        lb = logits.numpy().copy()
        model.set_sampling(do_sample=True, temperature=T, top_p=p, top_k=k, seed=SEED, bad_ids=BAD, begin_suppress_ids=BEGIN)
        x = _lib.DtkSamplingExt(min_p=min_p, epsilon_cutoff=eps)
        ref = {first: _oracle_row(logits, T, k, p, min_p, eps, first) for first in (True, False)}
        if tag == "eps .05 fallback":
            assert int((ref[False][0] > 0).sum()) == 1
            fell_back += 1
        if tag == "peaked":
            assert int((ref[False][0] > 0).sum()) == 1 and int(ref[False][0].argmax()) == V // 3
        if tag == "tie at the max":
            assert (ref[False][0] == (1 << 31)).nonzero().reshape(-1).tolist() == [17, V - 5]
        for n in range(16):
            qk, total, run = ref[n == 0]
            want = _oracle_token(run, total, n)
            model._check(model.lib.dtk_op_sample_ext(model._ctx, ptr(lb), V, n, C.byref(tok), ptr(probs), lp, C.byref(x)), "dtk_op_sample_ext")
            t = tok.value
            assert t == want, (V, tag, n, t, want)
            rp = (qk.double() / float(total)).float().numpy()
            assert int(((probs > 0) ^ (rp > 0)).sum()) == 0, (V, tag, n, "kept sets differ")
            assert np.allclose(probs, rp, rtol=1e-5, atol=1e-9), (V, tag, n)
            slp = math.log(int(qk[t]) / total)
            assert abs(lp[1] - slp) <= 1e-6 * abs(slp) if slp != 0.0 else lp[1] == 0.0, (V, tag, n, lp[1], slp)
            if n % 4 == 0:      # the kernels without the log-probability code: the same token
                model._check(model.lib.dtk_op_sample_ext(model._ctx, ptr(lb), V, n, C.byref(tok2), None, None, C.byref(x)), "dtk_op_sample_ext")
                assert tok2.value == t, (V, tag, n)
            model._check(model.lib.dtk_op_sample_lp(model._ctx, ptr(lb), V, n, C.byref(tok2), None, lp2), "dtk_op_sample_lp")
            if tok2.value == t:
                same_tok += 1
                assert bytes(C.c_float(lp[0])) == bytes(C.c_float(lp2[0])), (V, tag, n)
            else:               # another token: its own z against the same logsumexp (the bound of tests/test_gpu_logprobs.py)
                assert abs(lp[0] - float(torch.log_softmax(logits.double(), 0)[t])) <= 2e-5, (V, tag, n)
    print(f"op_sample_ext V={V} ({FAMILIES[V]}): 8 rows x 16 draws exact; {same_tok} draws chose dtk_op_sample_lp's token")
    # (the peaked row: its maximum holds all but ~V * e^-30 of the mass, so the plain sampler's top-p 0.95 keeps it alone as well)
    assert fell_back == 1 and same_tok >= 16
    # the ranges: DTK_ERR_ARG, nothing launched
    lb = np.zeros(8, dtype=np.float32)
    for bad in (_lib.DtkSamplingExt(min_p=-0.1), _lib.DtkSamplingExt(min_p=1.5), _lib.DtkSamplingExt(epsilon_cutoff=1.0),
                _lib.DtkSamplingExt(min_p=float("nan")), _lib.DtkSamplingExt(epsilon_cutoff=float("nan"))):
        assert model.lib.dtk_op_sample_ext(model._ctx, ptr(lb), 8, 0, C.byref(tok), None, None, C.byref(bad)) == -1
        assert model.lib.dtk_set_sampling_ext(model._ctx, C.byref(bad)) == -1


@pytest.mark.parametrize("V", list(FAMILIES), ids=[f"{v}-{k}" for v, k in FAMILIES.items()])
def test_off_means_off(big, V):
    """ext 0 / 0: the tokens, the probabilities and the pairs of dtk_op_sample_lp, bit for bit"""
    model = big
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    logits = rb(torch.randn(V, generator=torch.Generator().manual_seed(V + 1)) * 4)
    lb = logits.numpy().copy()
    off = _lib.DtkSamplingExt()
    tok, tok2, lp, lp2 = C.c_int64(), C.c_int64(), (C.c_float * 2)(), (C.c_float * 2)()
    p1, p2 = np.empty(V, dtype=np.float32), np.empty(V, dtype=np.float32)
    for T, k, p in ((0.8, V - 1 if V == 32769 else 0, 0.95), (1.3, 50, 1.0)):
        model.set_sampling(do_sample=True, temperature=T, top_p=p, top_k=k, seed=SEED, bad_ids=BAD, begin_suppress_ids=BEGIN)
        for n in range(8):
            model._check(model.lib.dtk_op_sample_ext(model._ctx, ptr(lb), V, n, C.byref(tok), ptr(p1), lp, C.byref(off)), "dtk_op_sample_ext")
            model._check(model.lib.dtk_op_sample_lp(model._ctx, ptr(lb), V, n, C.byref(tok2), ptr(p2), lp2), "dtk_op_sample_lp")
            assert tok.value == tok2.value and p1.tobytes() == p2.tobytes() and bytes(lp) == bytes(lp2), (V, T, k, n)
            assert tok.value == sampling.draw(logits, T, k, p, SEED, n, BAD, BEGIN, n == 0)[0]
    # a context whose configuration carries values, then a plain dtk_set_sampling: back to 0 / 0
    model.set_sampling(do_sample=True, temperature=1.0, seed=SEED, min_p=0.5)
    model._check(model.lib.dtk_op_sample_lp(model._ctx, ptr(lb), V, 3, C.byref(tok), None, lp), "dtk_op_sample_lp")
    assert tok.value == trunc_oracle.draw(logits, 1.0, 0, 1.0, SEED, 3, min_p=0.5)[0]
    model.set_sampling(do_sample=True, temperature=1.0, seed=SEED)
    model._check(model.lib.dtk_op_sample_lp(model._ctx, ptr(lb), V, 3, C.byref(tok), None, lp), "dtk_op_sample_lp")
    assert tok.value == sampling.draw(logits, 1.0, 0, 1.0, SEED, 3)[0]


# ------------------------------------------------------------------------------------------ one sequence, end to end
# (min_p 0.1, eps 3e-4) on the toy model's 512 near-flat logits (max - median ~ 1, p_max ~ 4e-3) keeps every token, and at 40 000 tokens
# (p_max ~ 1e-4 < eps) leaves the arg-max alone at every step: the third case is the toy model under a pair that cuts into its rows
@pytest.mark.parametrize("name,min_p,eps", [("detikzify-tiny", 0.1, 3e-4), ("tiny-v2-40000", 0.1, 3e-4), ("detikzify-tiny", 0.5, 3e-3)])
def test_generate_is_the_oracle_draw_over_the_device_logits(name, min_p, eps):
    """24 tokens of generate(min_p, epsilon_cutoff) == the tokens of the same steps driven by hand, each of which is the oracle's draw
    over the logits row the device sampled from (k_sample_fast on the toy vocabulary, the multi-block chain at 40 000)"""
    GEN = dict(do_sample=True, temperature=1.2, top_k=0, min_p=min_p, epsilon_cutoff=eps)
    if name == "detikzify-tiny":
        from detikzify_amd.model import load
        model, proc = load(name, synthetic=1234)
        enc = proc(images=sketch_image(2, 96), return_tensors="pt")
        ids, px, img = enc.input_ids[0], enc.pixel_values, TINY.image_token_id
    else:
        model = _bigvocab()
        cfg = model.config
        ids = torch.tensor([cfg.image_token_id] * cfg.num_patches + [77, 30123, 9])
        px, img = torch.zeros(1, 3, cfg.vit_image, cfg.vit_image), cfg.image_token_id
    out = model.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=24, eos_token_id=-1, bad_words_ids=[[img]], seed=31, **GEN)
    new = out[0, ids.numel():].tolist()
    assert len(new) == 24
    plain = model.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=24, eos_token_id=-1, bad_words_ids=[[img]], seed=31,
                           do_sample=True, temperature=1.2, top_k=0)
    model.set_sampling(do_sample=True, temperature=1.2, seed=31, bad_ids=[img], min_p=min_p, epsilon_cutoff=eps)
    model.prefill(ids, px)
    dropped = 0
    for n in range(24):
        row = model.get_logits()
        model.decode_launch()
        tok = model.decode_wait()
        want, probs, _ = trunc_oracle.draw(row, 1.2, 0, 1.0, 31, n, min_p, eps, [img])
        assert tok == want == new[n], (name, n, tok, want, new[n])
        z, q = sampling.integer_masses(row, 1.2, [img])
        dropped += int((q > 0).sum()) - int((probs > 0).sum())
    print(f"{name}: last row: max - median logit {float(row.max() - row.median()):.3f}, p_max {float(torch.softmax(row / 1.2, 0).max()):.2e}")
    print(f"{name}: 24 tokens exact; min_p / epsilon removed {dropped / 24:.0f} tokens per step; "
          f"{sum(a != b for a, b in zip(new, plain[0, ids.numel():].tolist()))} of 24 tokens differ from the run without them")
    del model
    gc.collect()


# ------------------------------------------------------------------------------------------ batched steps
PAIRS = [(0.1, 3e-4), (0.5, 0.0), (0.0, 0.0), (0.0, 3e-3)]       # slot s decodes under PAIRS[s]
STEPS = 12


def _prompts(proc, n):
    enc = proc(images=sketch_image(5, 96), return_tensors="pt")
    base, px = enc.input_ids[0], enc.pixel_values
    return [torch.cat([base, torch.tensor([20 + 3 * s, 41 + s][: 1 + s % 2], dtype=torch.int64)]) for s in range(n)], px


def _drive(model, prompts, px, slots, check):
    """STEPS batched steps of `slots` driven from the host; check: every token against the oracle's draw over the slot's own logits"""
    for s in slots:
        mp, eps = PAIRS[s]
        model.set_sampling(slot=s, do_sample=True, temperature=1.2, seed=900 + s, bad_ids=[TINY.image_token_id], min_p=mp, epsilon_cutoff=eps)
        model.prefill(prompts[s], px, slot=s)
    toks = {s: [] for s in slots}
    for n in range(STEPS):
        rows = {s: model.get_logits_slot(s) for s in slots} if check else {}
        model.decode_batch_launch(slots)
        t = model.decode_batch_wait()
        for s in slots:
            if check:
                want, probs, _ = trunc_oracle.draw(rows[s], 1.2, 0, 1.0, 900 + s, n, PAIRS[s][0], PAIRS[s][1], [TINY.image_token_id])
                assert t[s] == want, (s, n, t[s], want)
                if n == STEPS - 1:
                    print(f"slot {s} {PAIRS[s]}: keeps {int((probs > 0).sum())} of {probs.numel()} tokens at the last step")
            toks[s].append(int(t[s]))
    return toks


@pytest.fixture(scope="module", params=[5, 17], ids=["mv-4", "mfma-16"])
def batched(request):
    """detikzify-tiny with 5 slots (slots 0..3 decode with the multi-vector kernels) and with 17 (one MFMA column tile)"""
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny", synthetic=1234, batch_slots=request.param)
    assert model.max_decode_slots() == (4 if request.param == 5 else 16)
    prompts, px = _prompts(proc, 4)
    hand = _drive(model, prompts, px, [0, 1, 2, 3], check=True)       # (before anything switches the log-probabilities on)
    yield model, prompts, px, hand
    del model
    gc.collect()


def test_slots_with_their_own_pairs_are_exact_and_as_alone(batched):
    model, prompts, px, hand = batched
    for s in range(4):
        assert _drive(model, prompts, px, [s], check=False)[s] == hand[s], s
    # the pair matters: slot 2 (0 / 0) is the plain sampler's sequence, and some other slot's is not what it would be without its pair
    plain = {}
    for s in range(4):
        model.set_sampling(slot=s, do_sample=True, temperature=1.2, seed=900 + s, bad_ids=[TINY.image_token_id])
        model.prefill(prompts[s], px, slot=s)
    for n in range(STEPS):
        model.decode_batch_launch([0, 1, 2, 3])
        t = model.decode_batch_wait()
        for s in range(4):
            plain.setdefault(s, []).append(int(t[s]))
    assert plain[2] == hand[2]
    assert any(plain[s] != hand[s] for s in (0, 1, 3))


@pytest.mark.parametrize("engine", ["native", "python"])
def test_engines_carry_the_pairs_with_the_joins(batched, engine):
    """four sequences with their own pairs through either engine (one of them with return_logprobs): the tokens of the same slots driven
    by hand, which the fixture checked against the oracle"""
    from detikzify_amd.infer.batching import BatchEngine
    from detikzify_amd.infer.engine import NativeBatchEngine
    model, prompts, px, hand = batched
    model.enable_logprobs()
    eng = (NativeBatchEngine if engine == "native" else BatchEngine)(model, max_batch=4, share_prefix=False, resume_in_place=False)
    got, errs = {}, []

    def run(s):
        try:
            mp, eps = PAIRS[s]
            got[s] = model.generate(input_ids=prompts[s][None], pixel_values=px, max_new_tokens=STEPS, eos_token_id=-1, seed=900 + s,
                                    bad_words_ids=[[TINY.image_token_id]], do_sample=True, temperature=1.2, top_k=0, min_p=mp, epsilon_cutoff=eps,
                                    return_logprobs=(s == 0))
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    try:
        ths = [threading.Thread(target=run, args=(s,)) for s in range(4)]
        [t.start() for t in ths]
        [t.join(timeout=120) for t in ths]
        assert not any(t.is_alive() for t in ths) and not errs, errs[:1]
        # the same slots again without values: a join without them leaves nothing of the previous sequence's pair behind
        again = model.generate(input_ids=prompts[1][None], pixel_values=px, max_new_tokens=STEPS, eos_token_id=-1, seed=901,
                               bad_words_ids=[[TINY.image_token_id]], do_sample=True, temperature=1.2, top_k=0)
        again_mp = model.generate(input_ids=prompts[1][None], pixel_values=px, max_new_tokens=STEPS, eos_token_id=-1, seed=901,
                                  bad_words_ids=[[TINY.image_token_id]], do_sample=True, temperature=1.2, top_k=0, min_p=0.5)
    finally:
        eng.close()
    T = [p.numel() for p in prompts]
    for s in range(4):
        seq = got[s].sequences if s == 0 else got[s]
        assert seq[0, T[s]:].tolist() == hand[s], (engine, s)
    out = got[0]
    assert out.sample_logprobs.shape == (1, STEPS) and bool(torch.isfinite(out.sample_logprobs).all()) and bool((out.sample_logprobs <= 0).all())
    assert again_mp[0, T[1]:].tolist() == hand[1]
    plain1 = again[0, T[1]:].tolist()
    model.set_sampling(slot=1, do_sample=True, temperature=1.2, seed=901, bad_ids=[TINY.image_token_id])
    model.prefill(prompts[1], px, slot=1)
    ref = []
    for n in range(STEPS):
        model.decode_batch_launch([1])
        ref.append(int(model.decode_batch_wait()[1]))
    assert plain1 == ref
