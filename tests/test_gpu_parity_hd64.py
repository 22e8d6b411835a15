"""
head_dim 64 on the GPU (-m gpu): the TinyLlama decoder (nllg/detikzify-tl-1.1b: 32 query / 4 kv heads of 64) through the C ABI
against the CPU oracle.  The toy preset detikzify-tiny-tl (8 query heads of 64 over ONE kv head: G = 8, the same toy ViT as
detikzify-tiny) covers every single-sequence path in seconds with the criteria of tests/test_gpu_parity.py; the full-size
model is checked once against the oracle on a text prompt and for incremental == batched.
"""
import ctypes as C
import gc
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sampling
from oracle.llama import LlamaOracle, attention, rope_tables
from oracle.model import DetikzifyOracle
from oracle.ops import bits_to_f32, f32_to_bits, rb
from oracle.synth import synth_bits, tensor_specs
from tests.helpers import ENVELOPE, SLACK_LOGITS, gap_histogram, rel_l2, sketch_image, top2_gap_ulps

TL_TINY_NAME = "detikzify-tiny-tl"
SEED = 1234


def _preset(name, **over):
    from detikzify_amd.model.config import preset
    c = preset(name)
    for k, v in over.items():
        setattr(c, k, v)
    return c


TL_TINY = _preset(TL_TINY_NAME, max_positions=512)      # 512 positions: contexts that wrap the attention tiles around the splits
TL_TINY_CFG = TL_TINY.oracle_dict()


def device_weights(model, cfg, only=None):
    """every tensor the oracle needs (`only`: names with these prefixes), read back from the device (rope tables as [T][hd / 2])"""
    out = {}
    for name, shape, _, _ in tensor_specs(cfg):
        if only is not None and not name.startswith(only):
            continue
        if name.startswith("rope."):
            shape = (cfg["max_positions"], cfg["head_dim"] // 2)
        out[name] = model.read_tensor(name).float().reshape(shape)
    return out


@pytest.fixture(scope="module")
def tiny_tl():
    from detikzify_amd.model import load
    model, proc = load(TL_TINY_NAME, synthetic=SEED, max_positions=512)
    assert model.config.head_dim == 64 and model.config.num_kv_heads == 1
    return model, proc


@pytest.fixture(scope="module")
def tl_oracle(tiny_tl):
    model, _ = tiny_tl
    return DetikzifyOracle(TL_TINY_CFG, device_weights(model, TL_TINY_CFG), precision="bf16")


def run_greedy(model, ids, px, n, graph=1):
    model.set_graph_mode(graph)
    out = model.generate(input_ids=ids[None], pixel_values=px, do_sample=False, max_new_tokens=n,
                         bad_words_ids=[[model.config.image_token_id]], begin_suppress_tokens=[2], eos_token_id=-1)
    model.set_graph_mode(1)
    return out[0, ids.numel():].tolist()


def check_teacher_forced(oracle, logits, toks, img_tok=1, eos=2, max_flips=4):
    """greedy tokens identical to the oracle's except where its top-2 gap is within 2 bf16 ulps of the top logit"""
    flips = 0
    for i, t in enumerate(toks):
        rt = sampling.greedy(logits, [img_tok], [eos], i == 0)
        if rt != t:
            top2 = torch.topk(sampling.mask_scores(logits, [img_tok], [eos], i == 0), 2)[0]
            assert float(top2[0] - top2[1]) <= 2 * float(top2[0].abs()) * 2.0 ** -7 + 1e-6, (i, t, rt)
            flips += 1
        logits = oracle.step(t)
    assert flips <= max_flips, flips
    return flips


def tiny_prompt(proc, seed, extra=()):
    enc = proc(images=sketch_image(seed, 96), return_tensors="pt")
    ids = enc.input_ids[0]
    if len(extra):
        ids = torch.cat([ids, torch.as_tensor(extra, dtype=torch.int64)])
    return ids, enc.pixel_values


# ------------------------------------------------------------------------------------------ toy model, head_dim 64, G = 8
def test_tl_weights_and_rope_tables(tiny_tl):
    model, _ = tiny_tl
    for tag, (name, shape, scale, offset) in enumerate(tensor_specs(TL_TINY_CFG)):
        if name.startswith("rope.") or not (name.startswith("model.layers.1.") or name in ("lm_head.weight", "model.embed_tokens.weight")):
            continue
        got = f32_to_bits(model.read_tensor(name).float())
        assert np.array_equal(got, synth_bits(SEED, tag, int(np.prod(shape)), scale, offset)), name
    cos, sin = rope_tables(64, TL_TINY.rope_theta, TL_TINY.rope_factor, TL_TINY.max_positions)
    assert torch.equal(model.read_tensor("rope.cos").float().view(-1, 32), cos)
    assert torch.equal(model.read_tensor("rope.sin").float().view(-1, 32), sin)


def test_tl_prefill_logits(tiny_tl, tl_oracle):
    model, proc = tiny_tl
    ids, px = tiny_prompt(proc, 1, [70, 300, 41, 7])
    lo = model.prefill(ids, px, return_logits=True)
    ref = tl_oracle.prefill(ids, px[0])
    truth = DetikzifyOracle(TL_TINY_CFG, tl_oracle.w, precision="fp32").prefill(ids, px[0])
    r, e_dev, e_orc = rel_l2(lo, ref), rel_l2(lo, truth), rel_l2(ref, truth)
    print(f"hd64 prefill logits rel_l2 {r:.2e}; vs fp32 oracle: device {e_dev:.2e}, bf16 oracle {e_orc:.2e}")
    assert r < 1e-2 and e_dev < ENVELOPE * e_orc + SLACK_LOGITS and torch.isfinite(lo).all()
    t = torch.tensor([5, 9, 100, 44, 3, 8])
    assert rel_l2(model.prefill(t, None, return_logits=True), tl_oracle.prefill(t, None)) < 1e-2


def test_tl_greedy_token_identity_and_decode_logits(tiny_tl, tl_oracle):
    model, proc = tiny_tl
    ids, px = tiny_prompt(proc, 2)
    toks = run_greedy(model, ids, px, 48)
    flips = check_teacher_forced(tl_oracle, tl_oracle.prefill(ids, px[0]), toks)
    ids, px = tiny_prompt(proc, 3)
    model.set_sampling(do_sample=False, bad_ids=[1], begin_suppress_ids=[2])
    model.prefill(ids, px)
    ref = tl_oracle.prefill(ids, px[0])
    worst = rel_l2(model.get_logits(), ref)
    for _ in range(20):
        model.decode_launch()
        ref = tl_oracle.step(model.decode_wait())
        worst = max(worst, rel_l2(model.get_logits(), ref))
    print(f"hd64 greedy: {flips} near-tie flips in 48 tokens; decode logits worst rel_l2 {worst:.2e}")
    assert worst < 1e-2 and model.context_len() == ids.numel() + 20


def test_tl_sampled_draws_match_oracle(tiny_tl):
    model, proc = tiny_tl
    ids, px = tiny_prompt(proc, 6)
    kw = dict(do_sample=True, temperature=0.8, top_p=0.95, top_k=0, seed=99, max_new_tokens=32,
              bad_words_ids=[[1]], begin_suppress_tokens=[2], eos_token_id=-1)
    a = model.generate(input_ids=ids[None], pixel_values=px, **kw)[0, ids.numel():].tolist()
    assert a == model.generate(input_ids=ids[None], pixel_values=px, **kw)[0, ids.numel():].tolist() and len(set(a)) > 8
    model.set_sampling(do_sample=True, temperature=0.8, top_p=0.95, top_k=0, seed=99, bad_ids=[1], begin_suppress_ids=[2])
    model.prefill(ids, px)
    for i in range(32):
        lg = model.get_logits()
        model.decode_launch()
        t = model.decode_wait()
        rt, _ = sampling.draw(lg, 0.8, 0, 0.95, 99, i, [1], [2], i == 0)
        assert t == rt == a[i], f"draw {i}: device {t}, oracle {rt}, generate() {a[i]}"


def test_tl_graph_replay_equals_plain_launches(tiny_tl):
    model, proc = tiny_tl
    ids, px = tiny_prompt(proc, 4)
    assert run_greedy(model, ids, px, 40, graph=1) == run_greedy(model, ids, px, 40, graph=0)


def test_tl_attention_variants_agree_and_unsupported_are_refused(tiny_tl):
    """the tile-interleaved decode attention at hd 64 (8 lanes per 128-byte K/V row, 8 row groups per wave): 256 / 512 / 1024
    threads x 1..16 splits x own-kernel / consumer-side combine — identical greedy tokens, logits within the single-op bound.
    The contiguous-split kernels (attn_threads 0) have no hd-64 form and are refused."""
    model, proc = tiny_tl
    ids, px = tiny_prompt(proc, 9)
    outs, logs = {}, {}
    try:
        for threads in (256, 512, 1024):
            for splits in (1, 2, 4, 16):
                for combine in (2, 0):
                    model.set_option("attn_threads", threads)
                    model.set_option("attn_splits", splits)
                    model.set_option("attn_combine", combine)
                    key = (threads, splits, combine)
                    outs[key] = run_greedy(model, ids, px, 40)
                    logs[key] = model.get_logits()
        with pytest.raises(Exception, match="head_dim-64"):
            model.set_option("attn_threads", 0)
    finally:
        for k, v in dict(attn_combine=0, attn_threads=512, attn_splits=4).items():
            model.set_option(k, v)
    ref = (512, 4, 0)
    for key in outs:
        assert outs[key] == outs[ref], key
        assert rel_l2(logs[key], logs[ref]) < 5e-3, key


def test_tl_long_context_tiles_wrap_around(tiny_tl, tl_oracle):
    """contexts of 312..336 keys: one block walks several 128- / 256-row tiles (tile t belongs to split t % S); every geometry
    gives the same tokens, and the default geometry tracks the oracle"""
    model, proc = tiny_tl
    ids, px = tiny_prompt(proc, 3, (torch.arange(20, 20 + 300) % 500 + 3).tolist())
    got = {}
    try:
        for threads, splits in ((512, 4), (256, 1), (256, 2), (512, 1), (1024, 1), (256, 16)):
            model.set_option("attn_threads", threads)
            model.set_option("attn_splits", splits)
            got[(threads, splits)] = (run_greedy(model, ids, px, 24), model.get_logits())
    finally:
        model.set_option("attn_threads", 512)
        model.set_option("attn_splits", 4)
    ref = got[(512, 4)]
    for key, (toks, lg) in got.items():
        assert toks == ref[0], key
        assert rel_l2(lg, ref[1]) < 5e-3, key
    check_teacher_forced(tl_oracle, tl_oracle.prefill(ids, px[0]), ref[0])


def test_tl_gemv_variants_agree(tiny_tl):
    """every tuned shape of the two decode GEMV roles whose layout is per head (q/k/v + RoPE + KV append; o_proj reducing the
    attention partials in its prologue) at hd 64: identical greedy tokens, logits within the single-op bound"""
    model, proc = tiny_tl
    ids, px = tiny_prompt(proc, 4)
    lib, ctx = model.lib, model._ctx
    base = run_greedy(model, ids, px, 24)
    base_logits = model.get_logits()
    EPI_QKV, O_PROJ_ATTN = 2, 6
    try:
        for v in range(0, 12):
            model._check(lib.dtk_set_gemv_variant(ctx, EPI_QKV, v), "dtk_set_gemv_variant")
            assert run_greedy(model, ids, px, 24) == base, ("qkv", v)
            assert rel_l2(model.get_logits(), base_logits) < 5e-3, ("qkv", v)
        model._check(lib.dtk_set_gemv_variant(ctx, EPI_QKV, 0), "dtk_set_gemv_variant")
        model.set_option("attn_combine", 0)
        for splits in (4, 2):
            model.set_option("attn_splits", splits)
            for v in range(0, 9):
                model._check(lib.dtk_set_gemv_variant(ctx, O_PROJ_ATTN, v), "dtk_set_gemv_variant")
                assert run_greedy(model, ids, px, 24) == base, ("o_proj+combine", splits, v)
                assert rel_l2(model.get_logits(), base_logits) < 5e-3, ("o_proj+combine", splits, v)
    finally:
        lib.dtk_set_gemv_variant(ctx, EPI_QKV, 0)
        lib.dtk_set_gemv_variant(ctx, O_PROJ_ATTN, 0)
        for k, v in dict(attn_combine=0, attn_threads=512, attn_splits=4).items():
            model.set_option(k, v)


def test_tl_prefix_image_reuse_and_tail_prefill_are_bit_identical(tiny_tl):
    model, proc = tiny_tl
    ids, px = tiny_prompt(proc, 5)
    first = run_greedy(model, ids, px, 30)
    cont = torch.cat([ids, torch.tensor(first[:11])])
    fresh = model.prefill(cont, px, return_logits=True, reuse=False)
    n_before = model.stats()["prefill_tokens"]
    reused = model.prefill(cont, px, return_logits=True, reuse=True)         # LCP with the cached ids: only the last token
    assert model.stats()["prefill_tokens"] - n_before <= 1
    assert torch.equal(reused, fresh)
    model.prefill(cont[:-5], px, reuse=False)
    assert torch.equal(model.prefill(cont, px, return_logits=True, reuse=True), fresh), "5-row tail behind the cached head"
    model.prefill(torch.tensor([5, 9, 100]), None, reuse=False)               # another sequence; the image stays cached
    assert torch.equal(model.prefill(cont, px, return_logits=True, reuse=True), fresh), "cached image features"


@pytest.mark.parametrize("name", [TL_TINY_NAME, "detikzify-tl-1.1b"])
def test_tl_prefill_kernel_switches_are_bit_identical(name, tiny_tl):
    """the prefill switches that must not change a bit, at hd 64.  The real width (2 layers, a 300-row text prompt) takes the
    sliced-K q/k/v role fused with RoPE + KV append (k_sk_rope_scatter<S, 64>) against Linear + k_rope_scatter<64>."""
    g = torch.Generator().manual_seed(11)
    if name == TL_TINY_NAME:
        model, proc = tiny_tl
        ids, px = tiny_prompt(proc, 2, torch.randint(10, 400, (9,), generator=g).tolist())
    else:
        from detikzify_amd.model.modeling import DetikzifyForCausalLM
        model = DetikzifyForCausalLM(_preset(name, layers=2, max_positions=512), 0)
        model.fill_synthetic(31)
        ids, px = torch.randint(10, 32000, (300,), generator=g), None
    base = model.prefill(ids, px, return_logits=True, reuse=False)
    try:
        for opt, val, back in (("gemm_sk_tile", 0, 2), ("gemm_sk_tile", 1, 2), ("gemm_wt", 0, 1), ("gemm_epi_direct", 1, 0),
                               ("qkv_rope_fused", 0, 1), ("swiglu_fused", 0, 1), ("sk_sl_min_rows", 8, 768), ("attn_impl", 2, 0)):
            model.set_option(opt, val)
            got = model.prefill(ids, px, return_logits=True, reuse=False)
            model.set_option(opt, back)
            assert torch.equal(got, base), f"{opt} = {val}"
        model.prefill(ids[:-5], px, reuse=False)
        assert torch.equal(model.prefill(ids, px, return_logits=True, reuse=True), base), "5-row tail behind the cached head"
        model.set_option("attn_impl", 1)          # the VALU kernel: another summation order, close
        r = rel_l2(model.prefill(ids, px, return_logits=True, reuse=False), base)
        assert r < 1e-2, r
    finally:
        for opt, back in (("gemm_sk_tile", 2), ("gemm_wt", 1), ("gemm_epi_direct", 0), ("qkv_rope_fused", 1), ("sk_sl_min_rows", 768),
                          ("swiglu_fused", 1), ("attn_impl", 0)):
            model.set_option(opt, back)
        if name != TL_TINY_NAME:
            del model
            gc.collect()


@pytest.mark.parametrize("H,Tq,Tk,causal,qoff", [(3, 5, 19, 1, 14), (2, 70, 70, 1, 0), (2, 130, 200, 1, 70), (2, 300, 300, 1, 0),
                                                 (2, 36, 36, 0, 0), (2, 100, 257, 0, 0)])
@pytest.mark.parametrize("impl", [1, 2])
def test_tl_op_attention_hd64(tiny_tl, H, Tq, Tk, causal, qoff, impl):
    """hd 64: impl 1 = VALU kernel, impl 2 = k_attention_mfma<64>; both against the fp32-probability oracle"""
    model, _ = tiny_tl
    hd = 64
    model.set_option("attn_impl", impl)
    g = torch.Generator().manual_seed(H * 7 + Tq + Tk)
    q = rb(torch.randn(H, Tq, hd, generator=g)); k = rb(torch.randn(H, Tk, hd, generator=g)); v = rb(torch.randn(H, Tk, hd, generator=g))
    ref = attention(q, k, v, hd ** -0.5, qoff if causal else None)
    out = np.empty((H, Tq, hd), dtype=np.uint16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    qb, kb, vb = (f32_to_bits(torch.as_tensor(t, dtype=torch.float32)) for t in (q, k, v))
    try:
        model._check(model.lib.dtk_op_attention(model._ctx, p(qb), p(kb), p(vb), H, Tq, Tk, hd, causal, qoff, p(out)), "dtk_op_attention")
    finally:
        model.set_option("attn_impl", 0)
    got = bits_to_f32(out).reshape(-1)
    want = rb(torch.as_tensor(ref, dtype=torch.float32)).reshape(-1)
    ulp = torch.clamp(want.abs(), min=1e-2 * float(want.abs().max()) + 1e-30) * 2.0 ** -7
    ulps, rl2 = float(((got - want).abs() / ulp).max()), rel_l2(got, want)
    print(f"attention impl{impl} hd64 H{H} {Tq}x{Tk} causal={causal}: max_ulp {ulps:.2f} rel_l2 {rl2:.2e}")
    assert rl2 < 2e-3 and ulps <= 4.01


def test_tl_fp8_weights_parity():
    """weight_format="fp8" at hd 64 (launch_gemv_f8: the q/k/v epilogue with per-row scales of the (i, i+32) pairs): exactly
    e4m3-representable effective weights, and the fp8 decode / prefill against the oracle on those weights with the bounds of the
    bf16 path"""
    from detikzify_amd.model import load
    m8, proc = load(TL_TINY_NAME, synthetic=SEED, weight_format="fp8")
    m16, _ = load(TL_TINY_NAME, synthetic=SEED)
    cfg = m8.config.oracle_dict()
    try:
        name = "model.layers.1.self_attn.k_proj.weight"
        kvd = TL_TINY.num_kv_heads * TL_TINY.head_dim
        w8, w16 = m8.read_tensor(name).float().view(kvd, TL_TINY.hidden), m16.read_tensor(name).float().view(kvd, TL_TINY.hidden)
        amax = w16.abs().amax(dim=1, keepdim=True)
        q = w8 / torch.exp2(torch.ceil(torch.log2(amax / 448.0)))
        assert torch.equal(q, q.to(torch.float8_e4m3fn).float())
        assert float(((w8 - w16).abs() / (amax + 1e-30)).max()) <= 2.0 ** -4 + 1e-6
        oracle = DetikzifyOracle(cfg, device_weights(m8, cfg), precision="bf16")
        ids, px = tiny_prompt(proc, 2)
        lo = m8.prefill(ids, px, return_logits=True)
        r = rel_l2(lo, oracle.prefill(ids, px[0]))
        shift = rel_l2(lo, m16.prefill(ids, px, return_logits=True))
        toks = run_greedy(m8, ids, px, 32)
        logits, flips, worst = oracle.prefill(ids, px[0]), 0, 0.0
        m8.set_sampling(do_sample=False, bad_ids=[1], begin_suppress_ids=[2])
        m8.prefill(ids, px)
        for i, t in enumerate(toks):
            rt = sampling.greedy(logits, [1], [2], i == 0)
            if rt != t:
                top2 = torch.topk(sampling.mask_scores(logits, [1], [2], i == 0), 2)[0]
                assert float(top2[0] - top2[1]) <= 2 * float(top2[0].abs()) * 2.0 ** -7 + 1e-6, (i, t, rt)
                flips += 1
            m8.decode_launch()
            assert m8.decode_wait() == t
            logits = oracle.step(t)
            worst = max(worst, rel_l2(m8.get_logits(), logits))
        print(f"hd64 fp8: prefill vs oracle {r:.2e}; decode worst {worst:.2e}; {flips} flips; quantisation shift {shift:.2e}")
        assert r < 1e-2 and worst < 1e-2 and flips <= 3
        assert 1e-3 < shift < 0.3
        assert m8.stats()["weight_bytes_per_token"] < 0.56 * m16.stats()["weight_bytes_per_token"]
    finally:
        del m8, m16
        gc.collect()


def test_tl_safetensors_checkpoint_in_tinyllama_layout(tmp_path, tiny_tl):
    """a TinyLlama-layout checkpoint (config.json without head_dim, num_key_value_heads < heads, no rope_scaling; q/k/v/o and
    MLP tensors under their HF names; the tower in vision_tower.safetensors) loads to the synthetic fill's weights bit for bit"""
    from safetensors.torch import save_file
    from detikzify_amd.model import load
    from oracle.synth import make_weights
    c = TL_TINY
    w = {k: v.to(torch.bfloat16) for k, v in make_weights(TL_TINY_CFG, SEED).items()}
    save_file({k: v for k, v in w.items() if not k.startswith("vision_model.")}, str(tmp_path / "model.safetensors"))
    save_file({k[len("vision_model."):]: v for k, v in w.items() if k.startswith("vision_model.")}, str(tmp_path / "vision_tower.safetensors"))
    cfgj = dict(hidden_size=c.hidden, num_hidden_layers=c.layers, num_attention_heads=c.heads, num_key_value_heads=c.num_kv_heads,
                intermediate_size=c.ffn, vocab_size=c.vocab, rms_norm_eps=c.rms_eps, rope_theta=c.rope_theta, rope_scaling=None,
                bos_token_id=1, eos_token_id=2, pad_token_id=0, patch_token_id=1, concat_patches=3, feature_layer=c.vit_feature_layer,
                model_max_length=c.max_positions, vit_dim=c.vit_dim, vit_depth=c.vit_depth, vit_heads=c.vit_heads, vit_mlp=c.vit_mlp,
                vit_patch=c.vit_patch, vit_image=c.vit_image, vit_gelu_tanh=c.vit_gelu_tanh, attn_splits=c.attn_splits,
                synthetic_tokenizer=True)
    (tmp_path / "config.json").write_text(json.dumps(cfgj))
    model, proc = load(str(tmp_path))
    try:
        assert model.config.head_dim == 64 and model.config.kv_heads == 1
        ref, _ = tiny_tl
        for name in ("model.layers.1.self_attn.k_proj.weight", "model.layers.0.self_attn.v_proj.weight", "model.layers.1.self_attn.q_proj.weight",
                     "model.layers.0.self_attn.o_proj.weight", "lm_head.weight", "vision_model.blocks.0.attn.qkv.weight"):
            assert torch.equal(model.read_tensor(name), ref.read_tensor(name)), name
        ids, px = tiny_prompt(proc, 4)
        assert run_greedy(model, ids, px, 24) == run_greedy(ref, ids, px, 24)
    finally:
        del model
        gc.collect()


def test_tl_generate_and_pipeline_end_to_end(tiny_tl):
    from detikzify_amd.infer import DetikzifyPipeline, SyntheticTikzDocument
    model, proc = tiny_tl
    ids, px = tiny_prompt(proc, 7)
    out = model.generate(input_ids=ids[None], pixel_values=px, do_sample=False, max_length=40,
                         bad_words_ids=[[1]], begin_suppress_tokens=[2], eos_token_id=-1)
    assert out.shape == (1, 40) and 1 not in out[0, ids.numel():].tolist()
    pipe = DetikzifyPipeline(model, proc, metric="model", document_class=SyntheticTikzDocument, max_length=60)
    img = sketch_image(8, 128)
    assert isinstance(pipe.sample(img).code, str)
    res = list(pipe.simulate(img, expansions=4))
    assert len(res) == 4 and all(-1.0 <= s <= 1.0 + 1e-6 for s, _ in res)


# ------------------------------------------------------------------------------------------ full size
def test_tl_1_1b_refuses_batched_slots_in_dtk_create():
    """the C library makes the loader's refusal itself (C callers): DTK_ERR_ARG before anything is allocated"""
    from detikzify_amd.model.modeling import DetikzifyForCausalLM
    with pytest.raises(Exception, match="head_dim-64"):
        DetikzifyForCausalLM(_preset("detikzify-tl-1.1b", batch_slots=16), 0)


def test_tl_1_1b_matches_cpu_oracle_and_incremental_equals_batched():
    """detikzify-tl-1.1b at full size (synthetic weights) against the CPU oracle on a 96-token text prompt (the tower is the
    unchanged so400m of the other v1 models): prefill logits no further from the fp32 oracle than the bf16 oracle (ENVELOPE),
    16 greedy tokens with flips only at the oracle's own near-ties, 12 sampled draws exact; then with an image prompt, logits
    after prefill(T) == prefill(T - 1) + one decode step within 6e-3 sqrt(L), graph replay == plain launches."""
    from detikzify_amd.model import load
    model, proc = load("detikzify-tl-1.1b", synthetic=SEED, max_positions=512)
    try:
        cfg = model.config.oracle_dict()
        w = {k: v for k, v in device_weights(model, cfg, only=("model.", "lm_head.", "rope.")).items() if "mm_projector" not in k}
        o16, o32 = LlamaOracle(cfg, w, precision="bf16"), LlamaOracle(cfg, w, precision="fp32")
        ids = torch.randint(3, 32000, (96,), generator=torch.Generator().manual_seed(3))
        ids[0] = 1
        dev = model.prefill(ids, None, return_logits=True)
        ref, truth = (o.logits(o.forward(o.embed(ids))[-1]) for o in (o16, o32))
        r, e_dev, e_orc = rel_l2(dev, ref), rel_l2(dev, truth), rel_l2(ref, truth)
        assert e_dev < ENVELOPE * e_orc + SLACK_LOGITS, (e_dev, e_orc)
        toks = run_greedy(model, ids, None, 16)
        logits, near_ties, gaps = ref, 0, []
        for i, t in enumerate(toks):
            gaps.append(top2_gap_ulps(logits, [1], [2], i == 0))
            if sampling.greedy(logits, [1], [2], i == 0) != t:
                assert gaps[-1] <= 2.0 + 1e-3, (i, t, gaps[-1])
                near_ties += 1
            logits = o16.logits(o16.forward(o16.embed(torch.tensor([t])))[-1])      # teacher-forced
        near_tie_steps = sum(g <= 2.0 + 1e-3 for g in gaps)
        assert near_ties <= (near_tie_steps + 1) // 2 + 1, (near_ties, gap_histogram(gaps))
        model.set_sampling(do_sample=True, temperature=0.8, top_p=0.95, top_k=0, seed=4242, bad_ids=[1], begin_suppress_ids=[2])
        model.prefill(ids, None)
        for i in range(12):
            lg = model.get_logits()
            model.decode_launch()
            t = model.decode_wait()
            rt, _ = sampling.draw(lg, 0.8, 0, 0.95, 4242, i, [1], [2], i == 0)
            assert t == rt, f"sampled draw {i}: device {t}, oracle {rt}"
        print(f"tl-1.1b: prefill logits dev-vs-bf16-oracle {r:.2e}, vs fp32: device {e_dev:.2e} oracle {e_orc:.2e}; greedy "
              f"{16 - near_ties}/16 identical ({near_ties} flips in {near_tie_steps} near-tie steps); 12 sampled draws exact")
        del o16, o32, w
        gc.collect()
        enc = proc(images=sketch_image(0, 224), return_tensors="pt")
        ids, px = enc.input_ids[0], enc.pixel_values
        assert ids.numel() == 243
        toks = run_greedy(model, ids, px, 24, graph=1)
        assert toks == run_greedy(model, ids, px, 24, graph=0) and 1 not in toks
        prefix = torch.cat([ids, torch.tensor(toks[:8])])
        model.set_sampling(do_sample=False, bad_ids=[1])
        model.prefill(prefix, px)
        model.decode_launch()
        t = model.decode_wait()
        inc = model.get_logits()
        batched = model.prefill(torch.cat([prefix, torch.tensor([t])]), px, return_logits=True)
        ri, bound = rel_l2(inc, batched), 6e-3 * model.config.layers ** 0.5
        print(f"tl-1.1b: incremental-vs-batched logits rel_l2 {ri:.2e} (bound {bound:.2e})")
        assert torch.isfinite(batched).all() and ri < bound
    finally:
        del model
        gc.collect()
