"""kv_format "mxfp8" at model level on the MI355X (detikzify-tiny): the batched and multi-vector decode steps read the rows that
decode steps wrote as MXFP8 from the shadow planes.

  * greedy steps inside the fp32 envelope of the kv8 oracle (tests/kv8_oracle.py: the rows >= kv8_from quantised at attention time),
    the rule of test_fp8_matrix_core_step_...: d < ENVELOPE * o + SLACK_MX with o the oracle's own distance from the fp32 plain oracle;
  * dtk_read_kv8: every decoded row of every layer is mx_quantise of the bf16 row beside it, bit for bit, and the rows below the
    boundary were never written (0xFF);
  * the boundary through fork, whole-source fork, resume inside and below the decoded range, and a prefill with prefix reuse;
  * a bf16 context has no boundary (DTK_ERR_STATE), dtk_create refuses what the header says it refuses;
  * the host stack on a kv8 context: a fixed-seed batch gives the same tokens under both engines, a guided pair of generate() agrees with
    its manual loop, and an fp8 model with act_fp8 = 1 (MXFP8 activations AND MXFP8 key/value rows: the out8 store of the KV8 kernels)
    stays inside the envelope of the oracle with both quantisers on."""
from __future__ import annotations

import ctypes as C
import gc

import pytest
import torch

from detikzify_amd import _lib
from oracle.llama import mx_quantise
from oracle.model import DetikzifyOracle
from tests.helpers import ENVELOPE, SLACK_MX, TINY_CFG, rel_l2
from tests.kv8_oracle import kv8_oracle
from tests.test_gpu_parity_mv import weights_from_device

pytestmark = pytest.mark.gpu
STEPS = 8
DTK_ERR_ARG, DTK_ERR_STATE = -1, -3          # include/dtk.h


def _load(batch_slots, kv_format="mxfp8"):
    from detikzify_amd.model import load
    return load("detikzify-tiny", synthetic=1234, batch_slots=batch_slots, kv_format=kv_format)[0]


def _prompts(seed, lengths):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in lengths:
        ids = torch.randint(3, TINY_CFG["vocab"] - 1, (n,), generator=g)
        ids[ids == TINY_CFG["image_token_id"]] = 5
        out.append(ids)
    return out


def _steps(model, slots, n):
    toks, logs = {s: [] for s in slots}, {s: [] for s in slots}
    for _ in range(n):
        model.decode_batch_launch(slots)
        out = model.decode_batch_wait()
        for s in slots:
            toks[s].append(int(out[s]))
            logs[s].append(model.get_logits_slot(s))
    return toks, logs


def _envelope(w, context, toks, logs, kv_from, label):
    """context: the ids the slot held before the steps; the oracles are teacher-forced on the device's tokens in one pass"""
    oq, ob, o32 = kv8_oracle(TINY_CFG, w, "bf16", kv_from), DetikzifyOracle(TINY_CFG, w, precision="bf16"), DetikzifyOracle(TINY_CFG, w, precision="fp32")
    for o in (oq, ob, o32):
        o.prefill(context, None)
    rq, rb_, truth = oq.extend(toks), ob.extend(toks), o32.extend(toks)
    worst = eq = eb = 0.0
    for i, lg in enumerate(logs):
        d, o = rel_l2(lg, truth[i]), rel_l2(rq[i], truth[i])
        print(f"{label} step {i}: device vs fp32 {d:.2e}, kv8 oracle vs fp32 {o:.2e}; device vs kv8 oracle {rel_l2(lg, rq[i]):.2e}, vs plain bf16 oracle {rel_l2(lg, rb_[i]):.2e}")
        assert d < ENVELOPE * o + SLACK_MX, (label, i, d, o)
        worst = max(worst, d / (ENVELOPE * o + SLACK_MX))
    return worst


def _shadow_is_the_quantised_master(model, slot, frm, length, layers=TINY_CFG["layers"], untouched=True):
    """rows [frm, length) of every layer: codes and scales == mx_quantise(bf16 row); rows below frm were never written (untouched =
    False: a slot that earlier sequences decoded in)"""
    for layer in range(layers):
        for which in (0, 1):
            codes, scales, rows = model.read_kv8(slot, layer, which, 0, length)
            wc, ws = mx_quantise(rows[:, frm:].float(), 32)
            assert torch.equal(codes[:, frm:], wc) and torch.equal(scales[:, frm:], ws), (slot, layer, which)
            assert not untouched or ((codes[:, :frm] == 0xFF).all() and (scales[:, :frm] == 0xFF).all()), (slot, layer, which)


@pytest.mark.parametrize("batch_slots", [4, 17, 65])
def test_kv8_steps_stay_inside_the_kv8_oracles_envelope(batch_slots):
    """the multi-vector step (4 slots), one tile (17) and four tiles with the prefix kernel on (65): three sequences of different
    prompt lengths take 8 greedy steps"""
    model = _load(batch_slots)
    try:
        assert model.kv_format == "mxfp8"
        w = weights_from_device(model, TINY_CFG)
        NS = model.max_decode_slots()
        slots = [0, NS // 2, NS - 1]
        prompts = _prompts(batch_slots, (9, 40, 23))
        for s, ids in zip(slots, prompts):
            model.set_sampling(do_sample=False, slot=s)
            model.prefill(ids, None, slot=s)
            assert model.kv8_from(s) == ids.numel()
        toks, logs = _steps(model, slots, STEPS)
        worst = 0.0
        for s, ids in zip(slots, prompts):
            worst = max(worst, _envelope(w, ids, toks[s], logs[s], ids.numel(), f"{batch_slots} slots, slot {s}"))
            assert model.kv8_from(s) == ids.numel()
            _shadow_is_the_quantised_master(model, s, ids.numel(), ids.numel() + STEPS)
        print(f"kv8 step, batch_slots {batch_slots}: worst ratio to the fp32 envelope {worst:.2f}")
    finally:
        del model
        gc.collect()


def test_kv8_boundary_follows_fork_resume_and_prefill():
    model = _load(17)
    try:
        w = weights_from_device(model, TINY_CFG)
        (ids,) = _prompts(7, (30,))
        for s in range(4):
            model.set_sampling(do_sample=False, slot=s)
        # slot 0: prefill, 4 steps -> rows [30, 34) are MXFP8 rows
        model.prefill(ids, None, slot=0)
        t0, l0 = _steps(model, [0], 4)
        assert model.kv8_from(0) == 30
        # fork of a prefix of slot 0 that ends inside its decoded range: the destination's rows are all bf16 rows (read from slot 0's
        # bf16 cache), then a reuse prefill of one more token and steps of its own
        seq0 = torch.cat([ids, torch.tensor(t0[0][:3])])                       # 33 tokens whose rows slot 0 holds
        model.kv_fork(0, 1, 32)
        assert model.kv8_from(1) == 32
        model.prefill(seq0, None, slot=1, reuse=True)
        assert model.kv8_from(1) == 33
        t1, l1 = _steps(model, [1], 3)
        _envelope(w, seq0, t1[1], l1[1], 33, "fork of a prefix")
        _shadow_is_the_quantised_master(model, 1, 33, 36)
        # whole-source fork that decodes at once: slot 2 prefilled, forked to 3 in full
        (ids2,) = _prompts(8, (21,))
        model.prefill(ids2, None, slot=2)
        model.kv_fork(2, 3, 21)
        assert model.kv8_from(3) == 21
        t3, l3 = _steps(model, [3], 3)
        _envelope(w, ids2, t3[3], l3[3], 21, "whole-source fork")
        # resume inside slot 0's decoded range: the boundary is kept, rows [30, 32) stay MXFP8 rows
        path = torch.cat([ids, torch.tensor(t0[0][:3])])                       # cache holds ids + 4 tokens; resume with 33 tokens: keeps 32 rows
        model.resume_slot(0, path)
        assert model.kv8_from(0) == 30
        tr, lr = _steps(model, [0], 3)
        assert tr[0][0] == int(path[-1])                                       # the forced token
        _envelope(w, path, tr[0][1:], lr[0][1:], 30, "resume inside the decoded range")
        # resume below it: the boundary drops to T - 1
        low = ids[:20]
        model.resume_slot(0, low)
        assert model.kv8_from(0) == 19
        tl, ll = _steps(model, [0], 3)
        _envelope(w, low, tl[0][1:], ll[0][1:], 19, "resume below the boundary")
        _shadow_is_the_quantised_master(model, 0, 19, 22)
        # prefill with prefix reuse into a slot that had decoded: every row counts as a prefill row again
        again = torch.cat([low, torch.tensor(tl[0][1:2]), torch.tensor([7, 9])])
        model.prefill(again, None, slot=0, reuse=True)
        assert model.kv8_from(0) == again.numel()
        tp, lp = _steps(model, [0], 2)
        _envelope(w, again, tp[0], lp[0], again.numel(), "prefill with reuse")
    finally:
        del model
        gc.collect()


def test_bf16_context_has_no_boundary_and_create_refuses_bad_formats():
    model = _load(4, kv_format="bf16")
    try:
        assert model.kv_format == "bf16"
        out = C.c_int(0)
        assert model.lib.dtk_kv8_info(model._ctx, 0, C.byref(out)) == DTK_ERR_STATE
        with pytest.raises(_lib.DtkError):
            model.kv8_from(0)
        lib = model.lib
        kd = model.config.kernel_dict()
        for fmt, slots in ((2, 4), (-1, 4), (1, 0)):
            cc = _lib.DtkConfig(**kd)
            cc.reserved[0], cc.reserved[4] = slots, fmt
            ctx = C.c_void_p()
            assert lib.dtk_create(C.byref(cc), model.hip_device, C.byref(ctx)) == DTK_ERR_ARG and not ctx.value, (fmt, slots)
    finally:
        del model
        gc.collect()


# ------------------------------------------------------------------------------------------ the host stack on a kv8 context
def test_kv8_fixed_seed_batch_gives_the_same_tokens_under_both_engines():
    """four prompts generated from four threads through the native run loop and through the Python-driven engine, each on a FRESH kv8
    context of 5 slots (the multi-vector family): the same tokens.  The engines reach the cache through prefill / fork / resume only, so
    the boundary follows them without their knowing of it.  Fresh contexts, because in a kv8 context HOW a slot came to hold a prompt is
    part of the numbers: a prompt resumed in place (dtk_resume_slot: row T - 1 is decoded again and becomes an MXFP8 row) and the same
    prompt prefilled (row T - 1 a bf16 row) differ by that row's quantisation, and an engine resumes whenever a slot's history allows."""
    import threading

    from detikzify_amd.model import load
    from tests.helpers import engines
    from tests.test_gpu_parity_mv import _prompts as image_prompts
    kw = dict(do_sample=True, temperature=0.8, top_p=0.95, top_k=0, max_new_tokens=24, bad_words_ids=[[1]], begin_suppress_tokens=[2],
              eos_token_id=-1)
    results = {}
    for Engine in engines():
        model, proc = load("detikzify-tiny", synthetic=1234, batch_slots=5, kv_format="mxfp8")
        try:
            prompts = image_prompts(proc)
            engine = Engine(model)
            try:
                res = [None] * 4

                def run(i):
                    ids, px = prompts[i]
                    res[i] = model.generate(input_ids=ids[None], pixel_values=px, seed=50 + i, **kw)[0].tolist()
                engine.expect(4, timeout=30.0)
                ths = [threading.Thread(target=run, args=(i,)) for i in range(4)]
                [t.start() for t in ths]
                [t.join(timeout=120) for t in ths]
                assert all(r is not None and len(r) == prompts[i][0].numel() + 24 for i, r in enumerate(res)), Engine.__name__
                results[Engine.__name__] = res
            finally:
                engine.close()
            # every slot decoded behind its prompt — 23 forwarded tokens at the least, and an engine that keeps steps in flight has
            # launched one or two more by the time the 24th token is read: MXFP8 rows, and the shadow is the quantised master
            lens = sorted(model.context_len_slot(s) - model.kv8_from(s) for s in range(4))
            assert all(23 <= n <= 26 for n in lens), (Engine.__name__, lens)
            for s in range(4):
                _shadow_is_the_quantised_master(model, s, model.kv8_from(s), model.context_len_slot(s))
        finally:
            del model
            gc.collect()
    a, b = results.values()
    for i in range(4):
        assert a[i] == b[i], (i, next(k for k in range(len(a[i])) if a[i][k] != b[i][k]))


def test_kv8_guided_pair_agrees_with_its_manual_loop():
    """generate(guidance_scale=...) on a 2-slot kv8 context: the pair's tokens and log-probabilities are those of the pair stepped by
    hand (tests/test_gpu_cfg.py::_pair_by_hand: both rows mixed by the op, the oracle's pick over the mixed row), run twice"""
    from detikzify_amd.model import load
    from tests.test_gpu_cfg import G, _pair_by_hand, _prompts as pair_prompts
    model, proc = load("detikzify-tiny", synthetic=1234, batch_slots=2, kv_format="mxfp8")
    try:
        model.enable_logprobs()
        ids, px, px2 = pair_prompts(proc)
        T, N = int(ids.numel()), 12
        cfg = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=7)
        GEN = dict(input_ids=ids[None], pixel_values=px, guidance_scale=G, negative_pixel_values=px2, max_new_tokens=N, return_logprobs=True,
                   bad_words_ids=[[TINY_CFG["image_token_id"]]], eos_token_id=-1, **cfg)
        a = model.generate(**GEN)
        b = model.generate(**GEN)
        new = a.sequences[0, T:].tolist()
        assert len(new) == N and torch.equal(a.sequences, b.sequences)
        assert a.logprobs.numpy().tobytes() == b.logprobs.numpy().tobytes()
        assert model.kv8_from(0) == T and model.kv8_from(1) == T and model.context_len_slot(0) > T
        hand, bits, _ = _pair_by_hand(model, 0, 1, ids, px, px2, cfg, steps=N)
        assert hand == new and b"".join(bits) == a.logprobs.numpy().tobytes()
        for s in (0, 1):
            _shadow_is_the_quantised_master(model, s, T, model.context_len_slot(s))
    finally:
        del model
        gc.collect()


def test_kv8_with_mxfp8_activations_stays_inside_the_envelope_of_both_quantisers():
    """two layers of the cl-7b width, fp8 weights, act_fp8 = 1 and kv_format mxfp8: the fp8 matrix-core step, whose KV8 attention
    instantiation stores its head outputs as MXFP8 (out8).  6 greedy steps of three sequences against the kv8 oracle with act_quant on,
    the rule of test_fp8_matrix_core_step_...; then the shadow against the bf16 rows beside it"""
    from detikzify_amd.model.config import preset
    from detikzify_amd.model.modeling import DetikzifyForCausalLM
    from tests.test_gpu_parity import weights_from_device as weights_skipping
    cfg_m = preset("detikzify-cl-7b")
    cfg_m.layers, cfg_m.max_positions, cfg_m.batch_slots, cfg_m.weight_format, cfg_m.kv_format = 2, 256, 17, "fp8", "mxfp8"
    model = DetikzifyForCausalLM(cfg_m, 0)
    try:
        model.fill_synthetic(4321)
        model.set_option("act_fp8", 1)
        cfg = model.config.oracle_dict()
        w = weights_skipping(model, cfg, skip_prefix="vision_model.")
        slots = [0, 9, 15]
        g = torch.Generator().manual_seed(17)
        prompts = []
        for n in (9, 40, 23):
            ids = torch.randint(3, cfg["vocab"] - 1, (n,), generator=g)
            prompts.append(ids[ids != cfg["image_token_id"]])
        for s, ids in zip(slots, prompts):
            model.set_sampling(do_sample=False, slot=s)
            model.prefill(ids, None, slot=s)
        toks, logs = {s: [] for s in slots}, {s: [] for s in slots}
        for _ in range(6):
            model.decode_batch_launch(slots)
            out = model.decode_batch_wait()
            assert model.stats()["last_batch_step_fp8_mfma"] == 1
            for s in slots:
                toks[s].append(int(out[s]))
                logs[s].append(model.get_logits_slot(s))
        worst = 0.0
        for s, ids in zip(slots, prompts):
            oq, o32 = kv8_oracle(cfg, w, "bf16", ids.numel()), DetikzifyOracle(cfg, w, precision="fp32")
            oq.prefill(ids, None); o32.prefill(ids, None)          # the prefill keeps bf16 activations
            oq.llm.act_quant = True
            rq, truth = oq.extend(toks[s]), o32.extend(toks[s])
            for i, lg in enumerate(logs[s]):
                d, o = rel_l2(lg, truth[i]), rel_l2(rq[i], truth[i])
                print(f"act_fp8 + kv8, slot {s} step {i}: device vs fp32 {d:.2e}, oracle with both quantisers vs fp32 {o:.2e}; device vs that oracle {rel_l2(lg, rq[i]):.2e}")
                assert d < ENVELOPE * o + SLACK_MX, (s, i, d, o)
                worst = max(worst, d / (ENVELOPE * o + SLACK_MX))
            assert model.kv8_from(s) == ids.numel()
            _shadow_is_the_quantised_master(model, s, ids.numel(), ids.numel() + 6, layers=2)
        print(f"act_fp8 + kv8, two layers of cl-7b: worst ratio to the fp32 envelope {worst:.2f}")
    finally:
        del model
        gc.collect()
