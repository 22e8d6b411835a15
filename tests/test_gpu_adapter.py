"""TikZero adapter (text conditioning) on the MI355X: the toy v2 model with a toy embedding LLaMA (hd 64, GQA G = 4) against the
CPU restatement in tests/adapter_oracle.py, the gated-residual GEMM epilogue against its rounding, and image-only bit-identity."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import sampling
from oracle.model import DetikzifyOracle
from oracle.synth import tensor_specs
from tests.adapter_oracle import AdapterOracle, embed_text
from tests.helpers import ENVELOPE, SLACK_LOGITS, SLACK_SMALL, TINY_V2, TINY_V2_CFG, rel_l2, sketch_image

pytestmark = pytest.mark.gpu

TEXT_VOCAB = 300      # the toy embedding model's vocabulary (config.adapter_preset)


def _load(every_n=1, seed=4321, adapter=True):
    from detikzify_amd.model import load
    return load("detikzify-tiny-v2", synthetic=seed, adapter=adapter, cross_attn_every_n_layers=every_n)


def _weights(model):
    w = {n: model.read_tensor(n).float().reshape(s) for n, s, _, _ in tensor_specs(TINY_V2_CFG)}
    for n in model.tensor_names():
        if n.startswith(("adapter.", "embedding_model.")):
            w[n] = model.read_tensor(n).float()
    return w


def _text(n, seed=0):
    return torch.randint(0, TEXT_VOCAB, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)


@pytest.fixture(scope="module")
def pair():
    return {n: _load(n) for n in (1, 2)}


def _pixels(proc):
    return proc(images=sketch_image(0, 84), return_tensors="pt").pixel_values[0]


@pytest.mark.parametrize("every_n", [1, 2])
@pytest.mark.parametrize("T_text", [1, 63, 64, 65, 512])
def test_text_conditioned_features(pair, every_n, T_text):
    model, proc = pair[every_n]
    w = _weights(model)
    acfg = model.adapter_config.oracle_dict()
    ids = _text(T_text, T_text)
    px = _pixels(proc)
    dev_img = None
    for pixels in (px, None):          # text + image, text only (the dummy input)
        dev = model.vit_encode(None if pixels is None else pixels[None], want_pooled=False, adapter_input_ids=ids)[0][0].float()
        dev_img = dev if pixels is not None else dev_img
        ref = AdapterOracle(TINY_V2_CFG, acfg, w, "bf16").features(pixels, ids)
        truth = AdapterOracle(TINY_V2_CFG, acfg, w, "fp32").features(pixels, ids)
        e_dev, e_orc = rel_l2(dev, truth), rel_l2(ref, truth)
        assert e_dev < ENVELOPE * e_orc + SLACK_SMALL, (pixels is None, e_dev, e_orc)
    plain = model.vit_encode(px[None], want_pooled=False)[0][0].float()
    assert rel_l2(dev_img, plain) > 1e-2      # the same pixels: the text changes the features (synthetic gates are non-zero)


def test_embedding_pass_gqa4_hd64(pair):
    model, _ = pair[1]
    w = _weights(model)
    acfg = model.adapter_config.oracle_dict()
    assert acfg["heads"] // acfg["kv_heads"] == 4 and acfg["head_dim"] == 64
    for T in (1, 65, 512):
        ids = _text(T, 7 + T)
        dev = model.embed_text(ids).float()
        e_dev = rel_l2(dev, embed_text(acfg, w, ids, "fp32"))
        e_orc = rel_l2(embed_text(acfg, w, ids, "bf16"), embed_text(acfg, w, ids, "fp32"))
        assert e_dev < ENVELOPE * e_orc + SLACK_SMALL, (T, e_dev, e_orc)


def _gated_emulation(A, W, b, R, g):
    acc = A.float() @ W.float().T + b.float()
    o = acc.to(torch.bfloat16).float()
    gs = torch.sigmoid(g.float()).to(torch.bfloat16).float()
    return (R.float() + (gs * o).to(torch.bfloat16).float()).to(torch.bfloat16).float()


@pytest.mark.parametrize("K", [1152, 4304])
def test_gated_residual_epilogue_every_gemm_switch(pair, K):
    import ctypes as C
    model, _ = pair[1]
    lib, ctx = model.lib, model._ctx
    M, N = 900, 1152
    gen = torch.Generator().manual_seed(K)
    A = (torch.randn(M, K, generator=gen) * 0.5).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=gen) * 0.02).to(torch.bfloat16)
    b = (torch.randn(N, generator=gen) * 0.1).to(torch.bfloat16)
    R = torch.randn(M, N, generator=gen).to(torch.bfloat16)
    g = torch.tensor([-0.8], dtype=torch.bfloat16)
    emu = _gated_emulation(A, W, b, R, g)
    ungated = (R.float() + (A.float() @ W.float().T + b.float()).to(torch.bfloat16).float()).to(torch.bfloat16).float()
    bits = lambda t: t.contiguous().view(torch.int16).numpy()
    a_, w_, b_, r_, g_ = bits(A), bits(W), bits(b), bits(R), bits(g)
    out = np.empty((M, N), dtype=np.int16)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    # (gemm_impl, gemm_tile, extra options): at M = 900, N = 1152 neither k_gemm_g3 (36 blocks < 128) nor k_gemm_glds (72 tiles < 160)
    # takes the shape by default — their thresholds are lowered so that each kernel (and g3's direct epilogue) really runs
    switches = [(3, 0, {}), (0, 0, {}), (0, 1, {}), (0, 2, {}), (0, 3, {}), (0, 4, {}), (0, 5, {}),
                (2, 0, {"gemm_glds_min_tiles": 1}), (4, 0, {"gemm_g3_min_blocks": 1}),
                (4, 0, {"gemm_g3_min_blocks": 1, "gemm_epi_direct": 1})]
    try:
        for impl, tile, extra in switches + [("naive", None, {})]:
            flags = 0
            if impl == "naive":
                flags = 256
            else:
                model.set_option("gemm_impl", impl)
                model.set_option("gemm_tile", tile)
                for k, v in extra.items():
                    model.set_option(k, v)
            rc = lib.dtk_op_gemm_gated(ctx, ptr(a_), ptr(w_), ptr(b_), ptr(r_), ptr(g_), M, N, K, flags, ptr(out))
            assert rc == 0, lib.dtk_last_error(ctx)
            dev = torch.from_numpy(out.copy()).view(torch.bfloat16).float()
            assert rel_l2(dev, emu) < 2e-3, (impl, tile, rel_l2(dev, emu))
            assert rel_l2(dev, ungated) > 2e-2, (impl, tile)       # the gate was applied
            for k in extra:
                model.set_option(k, {"gemm_glds_min_tiles": 160, "gemm_g3_min_blocks": 128, "gemm_epi_direct": 0}[k])
    finally:
        for k, v in (("gemm_impl", 3), ("gemm_tile", 0), ("gemm_glds_min_tiles", 160), ("gemm_g3_min_blocks", 128), ("gemm_epi_direct", 0)):
            model.set_option(k, v)


def test_image_only_bit_identical_with_and_without_adapter():
    plain, proc = _load(adapter=False)
    with_ad, _ = _load(2)
    px = _pixels(proc)
    enc = proc(images=sketch_image(0, 84), return_tensors="pt")
    kw = dict(do_sample=False, max_new_tokens=12, bad_words_ids=[[TINY_V2.image_token_id]], eos_token_id=-1)
    f0 = plain.vit_encode(px[None])
    t0 = plain.generate(input_ids=enc.input_ids, pixel_values=enc.pixel_values, **kw)
    for m in (with_ad, "unloaded"):
        if m == "unloaded":
            with_ad.vit_encode(px[None], adapter_input_ids=_text(9))       # a text-conditioned pass first: nothing of it may stay
            with_ad.unload_cross_attn_adapter()
            m = with_ad
        f1 = m.vit_encode(px[None])
        assert torch.equal(f0[0].view(torch.int16), f1[0].view(torch.int16)) and torch.equal(f0[1].view(torch.int16), f1[1].view(torch.int16))
        assert torch.equal(t0, m.generate(input_ids=enc.input_ids, pixel_values=enc.pixel_values, **kw))
    with pytest.raises(TypeError):
        with_ad.generate(input_ids=enc.input_ids, pixel_values=enc.pixel_values, adapter_input_ids=_text(3), **kw)


def test_text_conditioned_prefill_and_greedy_decode(pair):
    model, proc = pair[2]
    w = _weights(model)
    acfg = model.adapter_config.oracle_dict()
    ids_text = _text(40, 3)
    enc = proc(images=sketch_image(1, 84), return_tensors="pt")
    ids, px = enc.input_ids[0], enc.pixel_values
    feats = AdapterOracle(TINY_V2_CFG, acfg, w, "bf16").features(px[0], ids_text)
    feats32 = AdapterOracle(TINY_V2_CFG, acfg, w, "fp32").features(px[0], ids_text)
    main = {n: v for n, v in w.items() if not n.startswith(("adapter.", "embedding_model."))}
    oracle = DetikzifyOracle(TINY_V2_CFG, main, precision="bf16")
    logits = oracle.prefill(ids, px[0], vit_feats=feats)
    truth = DetikzifyOracle(TINY_V2_CFG, main, precision="fp32").prefill(ids, px[0], vit_feats=feats32)
    dev = model.prefill(ids, px, return_logits=True, adapter_input_ids=ids_text)
    e_dev, e_orc = rel_l2(dev, truth), rel_l2(logits, truth)
    assert e_dev < ENVELOPE * e_orc + SLACK_LOGITS, (e_dev, e_orc)
    plain = model.prefill(ids, px, return_logits=True)
    assert rel_l2(dev, plain) > 1e-3         # image-only prefill of the same pixels is another prefix
    bad = [TINY_V2.image_token_id]
    out = model.generate(input_ids=ids[None], pixel_values=px, do_sample=False, max_new_tokens=12, bad_words_ids=[bad],
                         eos_token_id=-1, adapter_input_ids=ids_text[None], adapter_attention_mask=torch.ones(1, 40, dtype=torch.int64))
    toks = out[0, ids.numel():].tolist()
    for i, t in enumerate(toks):
        rt = sampling.greedy(logits, bad, [], i == 0)
        if rt != t:
            top2 = torch.topk(sampling.mask_scores(logits, bad, [], i == 0), 2)[0]
            assert float(top2[0] - top2[1]) <= 2 * float(top2[0].abs()) * 2.0 ** -7 + 1e-6, (i, t, rt)
        logits = oracle.step(t)
    with pytest.raises(NotImplementedError):
        model.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=2, adapter_input_ids=ids_text[None],
                       adapter_attention_mask=torch.tensor([[1] * 39 + [0]]))


def test_prefix_cache_separates_texts(pair):
    model, proc = pair[1]
    enc = proc(images=sketch_image(2, 84), return_tensors="pt")
    ids, px = enc.input_ids[0], enc.pixel_values
    a = model.prefill(ids, px, return_logits=True, reuse=False, adapter_input_ids=_text(20, 1))
    b = model.prefill(ids, px, return_logits=True, reuse=False, adapter_input_ids=_text(20, 2))
    b_reused = model.prefill(ids, px, return_logits=True, reuse=True, adapter_input_ids=_text(20, 2))
    a_reused = model.prefill(ids, px, return_logits=True, reuse=True, adapter_input_ids=_text(20, 1))
    assert torch.equal(a, a_reused) and torch.equal(b, b_reused) and not torch.equal(a, b)


def test_pipeline_text_end_to_end(pair):
    """DetikzifyPipeline.sample(text=...) (text only: the dummy image) and simulate(image, text=..., expansions=4) with the
    text-conditioned SelfSim reward (ImageSim.update(text2=...))"""
    from detikzify_amd.evaluate.imagesim import ImageSim
    from detikzify_amd.infer import DetikzifyPipeline, SyntheticTikzDocument
    from detikzify_amd.model import AdapterProcessor
    model, proc = pair[1]
    assert isinstance(proc, AdapterProcessor)
    pipe = DetikzifyPipeline(model, proc, metric="model", document_class=SyntheticTikzDocument, max_length=12 + 40, compile_timeout=None)
    doc = pipe.sample(text="a red circle")
    assert isinstance(doc, SyntheticTikzDocument)
    image = sketch_image(3, 84)
    got = list(pipe.simulate(image, text="a red circle", expansions=4))
    assert len(got) == 4 and all(isinstance(float(score), float) for score, _ in got)
    # the reward's reference features are the text-conditioned tower's
    sim = ImageSim.from_detikzify(model, proc, preprocess=False)     # the same pixels as `px` below (no trim / expand)
    ids = torch.tensor(proc.tokenizer(text=["a red circle"])["input_ids"][0])
    px = proc(images=image, return_tensors="pt")["pixel_values"]
    want = model.vit_encode(px, want_pooled=False, adapter_input_ids=ids)[0][0]
    assert torch.equal(sim.get_vision_features(image, "a red circle").view(torch.int16), want.view(torch.int16))
    assert not torch.equal(sim.get_vision_features(image).view(torch.int16), want.view(torch.int16))
    sim.update(img1=image, img2=image, text2="a red circle")
    assert sim.compute() < 0.999


def test_full_size_v2_5_8b_adapter_features():
    """detikzify-v2.5-8b + a seeded Llama-3.2-1B adapter (every_n 1): text-conditioned features against ONE bf16 CPU reference pass"""
    from detikzify_amd.model import load
    model, proc = load("detikzify-v2.5-8b", synthetic=11, adapter=True)
    c = model.config
    w = {}
    for n in model.tensor_names():
        if n.startswith(("adapter.", "embedding_model.")):
            w[n] = model.read_tensor(n).float()
        elif n.startswith("vision_model.") and not n.startswith("vision_model.attn_pool."):
            w[n] = model.read_tensor(n).float()
    D, pk = c.vit_dim, 3 * c.vit_patch ** 2
    w["vision_model.patch_embed.proj.weight"] = w["vision_model.patch_embed.proj.weight"].reshape(D, pk)
    w["vision_model.pos_embed"] = w["vision_model.pos_embed"].reshape(-1, D)
    ids = torch.randint(0, model.adapter_config.vocab, (64,), generator=torch.Generator().manual_seed(5))
    px = proc(images=sketch_image(4, 420), return_tensors="pt")["pixel_values"]
    dev = model.vit_encode(px, want_pooled=False, adapter_input_ids=ids)[0][0].float()
    plain = model.vit_encode(px, want_pooled=False)[0][0].float()
    with torch.inference_mode():
        ref = AdapterOracle(c.oracle_dict(), model.adapter_config.oracle_dict(), w, "bf16").features(px[0], ids)
    assert rel_l2(dev, ref) < 3e-2, rel_l2(dev, ref)
    assert rel_l2(dev, ref) < 0.5 * rel_l2(plain, ref), (rel_l2(dev, ref), rel_l2(plain, ref))
