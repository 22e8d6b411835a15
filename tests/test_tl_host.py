"""detikzify-tl-1.1b (TinyLlama: head_dim 64, GQA 32 / 4) on the host side, no GPU: the presets, the config.json reader,
the loader's shape gate, and the oracle at head_dim 64 with G = 8 against the installed transformers LLaMA."""
import json

import pytest
import torch

from detikzify_amd.model import _require_supported
from detikzify_amd.model.config import DetikzifyConfig, preset
from oracle.llama import LlamaOracle
from oracle.synth import make_weights
from tests.helpers import rel_l2


def test_tl_preset_shapes():
    c = preset("detikzify-tl-1.1b")
    assert preset("nllg/detikzify-tl-1.1b") == c
    assert (c.hidden, c.layers, c.heads, c.num_kv_heads, c.head_dim, c.ffn) == (2048, 22, 32, 4, 64, 5632)
    assert c.hidden == c.heads * c.head_dim and c.heads // c.num_kv_heads == 8
    assert (c.rms_eps, c.rope_theta, c.rope_factor, c.rope_type) == (1e-5, 10000.0, 1.0, "linear")
    assert (c.vocab, c.bos_token_id, c.eos_token_id, c.pad_token_id, c.patch_token_id) == (32008, 1, 2, 32000, 1)
    assert c.vocab % 8 == 0 and c.pad_token_id == 32000           # <pad> appended to 32 000 entries, resized to a multiple of 8
    assert c.image_token_id == c.bos_token_id                     # v1: the patch token is BOS
    assert (c.vit_dim, c.vit_depth, c.vit_image, c.arch) == (1152, 27, 384, "v1")
    assert c.num_patches == 243


def test_tiny_tl_preset_is_head_dim_64_with_groups_of_8():
    c, t = preset("detikzify-tiny-tl"), preset("detikzify-tiny")
    assert (c.head_dim, c.heads, c.num_kv_heads, c.hidden, c.layers, c.attn_splits) == (64, 8, 1, 512, 2, 4)
    assert c.hidden == c.heads * c.head_dim
    for k in ("vit_dim", "vit_depth", "vit_heads", "vit_mlp", "vit_patch", "vit_image", "vit_feature_layer", "concat_patches"):
        assert getattr(c, k) == getattr(t, k), k
    d = c.oracle_dict()
    assert d["head_dim"] == 64 and d["kv_heads"] == 1


def test_from_hf_json_tinyllama_layout(tmp_path):
    """a TinyLlama-shaped config.json (no head_dim key, num_key_value_heads 4, no rope_scaling) -> hd 64, 4 kv heads, factor 1"""
    j = dict(architectures=["DetikzifyForCausalLM"], model_type="detikzify", hidden_size=2048, intermediate_size=5632,
             num_hidden_layers=22, num_attention_heads=32, num_key_value_heads=4, rms_norm_eps=1e-5, rope_theta=10000.0,
             rope_scaling=None, vocab_size=32008, bos_token_id=1, eos_token_id=2, pad_token_id=32000, max_position_embeddings=2048)
    (tmp_path / "config.json").write_text(json.dumps(j))
    c = DetikzifyConfig.from_hf_json(str(tmp_path / "config.json"))
    assert (c.head_dim, c.kv_heads, c.num_kv_heads, c.rope_factor, c.rope_type) == (64, 4, 4, 1.0, "linear")
    assert (c.hidden, c.layers, c.heads, c.ffn, c.vocab, c.pad_token_id) == (2048, 22, 32, 5632, 32008, 32000)
    _require_supported(c)


def test_require_supported_head_dims():
    c = preset("detikzify-tl-1.1b")
    _require_supported(c)                              # head_dim 64, one sequence per context
    c.batch_slots = 16
    with pytest.raises(NotImplementedError, match="no head_dim-64 kernels"):
        _require_supported(c)
    c = preset("detikzify-tiny-tl")
    _require_supported(c)
    c.batch_slots = 1
    with pytest.raises(NotImplementedError, match="batched decode slots"):
        _require_supported(c)
    c = preset("detikzify-ds-1.3b")
    c.batch_slots = 16
    _require_supported(c)                              # head_dim 128 keeps its slots
    c = preset("detikzify-tiny")
    c.head_dim, c.heads = 96, 2
    with pytest.raises(NotImplementedError, match="head_dim 96"):
        _require_supported(c)


def test_load_refuses_head_dim_64_with_slots_before_any_kernel():
    """the gate sits in front of the device: no library call is needed to get the refusal"""
    from detikzify_amd.model import load
    with pytest.raises(NotImplementedError, match="head_dim-64"):
        load("detikzify-tl-1.1b", synthetic=1, batch_slots=16)


def test_head_dim_64_gqa_oracle_matches_hf_llama():
    """the oracle's LLaMA at head_dim 64 with G = 8 (TinyLlama's 2048 width and 32 / 4 heads, 2 layers, a smaller vocab) on
    seeded synthetic weights against the installed HF LlamaForCausalLM in fp32: 24 prompt positions and 3 cached decode steps."""
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = dict(preset("detikzify-tl-1.1b").oracle_dict(), layers=2, vocab=4096, max_positions=64)
    assert cfg["head_dim"] == 64 and cfg["kv_heads"] == 4
    w = make_weights(cfg, 77, only_prefix="model.")
    w.update(make_weights(cfg, 77, only_prefix="lm_head"))
    hf = LlamaForCausalLM(LlamaConfig(
        hidden_size=cfg["hidden"], intermediate_size=cfg["ffn"], num_hidden_layers=2, num_attention_heads=cfg["heads"],
        num_key_value_heads=cfg["kv_heads"], head_dim=cfg["head_dim"], vocab_size=cfg["vocab"], rms_norm_eps=cfg["rms_eps"],
        max_position_embeddings=cfg["max_positions"], rope_theta=cfg["rope_theta"], rope_scaling=None, attention_bias=False,
        tie_word_embeddings=False, bos_token_id=1, eos_token_id=2, pad_token_id=0)).eval()
    sd = {k: v.float().contiguous() for k, v in w.items() if k in hf.state_dict()}
    assert set(sd) == set(hf.state_dict())
    hf.load_state_dict(sd, strict=True, assign=True)
    ids = torch.randint(3, cfg["vocab"], (1, 24), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        out = hf(input_ids=ids, use_cache=True)
        llm = LlamaOracle(cfg, w, precision="fp32")
        mine = llm.logits(llm.forward(llm.embed(ids[0])))
        assert rel_l2(mine, out.logits[0]) < 2e-5
        for tok in (17, 2048, 4095):
            out = hf(input_ids=torch.tensor([[tok]]), past_key_values=out.past_key_values, use_cache=True)
            assert rel_l2(llm.logits(llm.forward(llm.embed(torch.tensor([tok])))[-1]), out.logits[0, -1]) < 2e-5
