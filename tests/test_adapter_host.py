"""TikZero adapter, host side (no GPU): configuration, the adapter_* arguments, the (image, text) cache key, refusals."""
from __future__ import annotations

import json

import pytest
import torch

from detikzify_amd import _lib
from detikzify_amd.model import AdapterConfig, adapter_preset, load
from detikzify_amd.model.modeling import DetikzifyForCausalLM, adapter_text, text_key

LLAMA_3_2_1B = {"hidden_size": 2048, "num_hidden_layers": 16, "num_attention_heads": 32, "num_key_value_heads": 8, "head_dim": 64,
                "intermediate_size": 8192, "vocab_size": 128256, "rms_norm_eps": 1e-5, "rope_theta": 500000.0, "bos_token_id": 128000,
                "rope_scaling": {"rope_type": "llama3", "factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                 "original_max_position_embeddings": 8192}, "tie_word_embeddings": True}


def test_adapter_config_is_parsed(tmp_path):
    (tmp_path / "emb.json").write_text(json.dumps(LLAMA_3_2_1B))
    c = AdapterConfig.from_hf(str(tmp_path / "emb.json"))
    assert (c.hidden, c.layers, c.heads, c.kv_heads, c.head_dim, c.ffn, c.vocab) == (2048, 16, 32, 8, 64, 8192, 128256)
    assert (c.rope_type, c.rope_factor, c.rope_low_freq_factor, c.rope_high_freq_factor, c.rope_original_max_position) == \
        ("llama3", 32.0, 1.0, 4.0, 8192)
    assert c.every_n == 1 and c.text_max == 512 and c == AdapterConfig()
    (tmp_path / "adapter.json").write_text(json.dumps({"cross_attn_every_n_layers": 3}))
    assert AdapterConfig.from_hf(str(tmp_path / "emb.json"), str(tmp_path / "adapter.json"), every_n=2).every_n == 3
    assert AdapterConfig.from_hf(str(tmp_path / "emb.json"), str(tmp_path / "missing.json"), every_n=2).every_n == 2
    toy = adapter_preset("detikzify-tiny-v2", 2)
    assert toy.every_n == 2 and toy.heads // toy.kv_heads == 4 and toy.head_dim == 64


def test_adapter_config_struct_matches_the_library():
    import ctypes
    lib = _lib.load_library()
    assert lib.dtk_abi_version() == 7
    assert lib.dtk_abi_struct_size(11) == ctypes.sizeof(_lib.DtkAdapterConfig) == 18 * 4


def test_adapter_text_arguments():
    ids = torch.arange(5)[None]
    assert torch.equal(adapter_text(ids, torch.ones(1, 5)), torch.arange(5))
    with pytest.raises(NotImplementedError, match="padded"):
        adapter_text(ids, torch.tensor([[1, 1, 1, 0, 0]]))
    with pytest.raises(ValueError):
        adapter_text(torch.zeros(2, 5, dtype=torch.int64))


def test_generate_takes_adapter_arguments_only_with_an_adapter():
    m = object.__new__(DetikzifyForCausalLM)          # no context: both calls must be decided before the device is touched
    m._weights_ready = True
    for kw in (dict(adapter_input_ids=torch.arange(3)[None]), dict(adapter_attention_mask=torch.ones(1, 3))):
        with pytest.raises(TypeError, match="no adapter"):
            m.generate(input_ids=torch.arange(4)[None], max_new_tokens=2, **kw)
    m.adapter = object()
    with pytest.raises(NotImplementedError, match="padded"):
        m.generate(input_ids=torch.arange(4)[None], max_new_tokens=2, adapter_input_ids=torch.arange(3)[None],
                   adapter_attention_mask=torch.tensor([[1, 1, 0]]))


def test_prefix_cache_key_separates_texts():
    lib = _lib.load_library()
    img = 0x1234_5678_9ABC_DEF0
    a, b = text_key(torch.tensor([1, 2, 3])), text_key(torch.tensor([1, 2, 4]))
    assert a != b and a == text_key(torch.tensor([[1, 2, 3]]))
    ka, kb = lib.dtk_text_image_key(img, a), lib.dtk_text_image_key(img, b)
    assert ka != kb and ka not in (0, img) and ka == lib.dtk_text_image_key(img, a)
    assert lib.dtk_text_image_key(img + 1, a) != ka
    assert lib.dtk_text_image_key(0, a) == 0 and lib.dtk_text_image_key(img, 0) == 0      # an unknown key is never reused


def test_v1_tower_is_refused():
    with pytest.raises(ValueError, match="Couldn't locate vision encoder layers!"):
        load("detikzify-tiny", synthetic=1, adapter=True)


def test_missing_embedding_model_is_a_file_not_found(tmp_path):
    cfg = {"text_config": {"hidden_size": 512, "num_hidden_layers": 2, "num_attention_heads": 4, "num_key_value_heads": 2,
                           "intermediate_size": 688, "vocab_size": 640, "rope_theta": 500000.0, "bos_token_id": 1, "eos_token_id": 2},
           "vision_config": {"hidden_size": 144, "num_hidden_layers": 2, "num_attention_heads": 2, "intermediate_size": 304,
                             "image_size": 84, "patch_size": 14},
           "image_token_id": 5, "synthetic_tokenizer": True}
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    (tmp_path / "adapter").mkdir()
    (tmp_path / "adapter" / "model.safetensors").write_bytes(b"")
    with pytest.raises(FileNotFoundError, match="embedding model"):
        load(str(tmp_path))
    with pytest.raises(FileNotFoundError, match="embedding model"):
        load(str(tmp_path), embedding_model=str(tmp_path / "nowhere"))


def test_cpu_adapter_reference_matches_the_reference_module():
    """tests/adapter_oracle.py (fp32) against the reference's own CrossAttentionAdapter (tests/golden/make_adapter_golden.py)"""
    import numpy as np
    from pathlib import Path
    from tests.adapter_oracle import AdapterOracle
    d = np.load(Path(__file__).resolve().parent / "golden" / "adapter_tiny.npz")
    w = {k: torch.from_numpy(d[k]).reshape(-1) for k in d.files if k.startswith("adapter.")}
    vcfg = dict(vit_dim=64, vit_heads=2, vit_mlp=96, vit_depth=2, vit_ln_eps=1e-6, vit_gelu_tanh=1, vit_image=56, vit_feature_layer=1)
    o = AdapterOracle(vcfg, dict(every_n=1, hidden=48), w, "fp32")
    c = o._lin(torch.from_numpy(d["hidden"]), "adapter.connector", 64, 48)
    assert torch.allclose(c, torch.from_numpy(d["connected"]), atol=1e-6, rtol=1e-6)
    kv = o.cross_kv(c)
    x = torch.from_numpy(d["x"])
    for i in range(2):
        out, ref = o.cross_layer(x, i, kv), torch.from_numpy(d[f"out.{i}"])
        assert (out - ref).norm() / ref.norm() < 1e-6 and (out - x).norm() / x.norm() > 1e-2, i
    assert torch.equal(o.dummy_pixels(), w["adapter.dummy_input"].reshape(3, 56, 56).clamp(-1, 1))


def test_adapter_processor_outputs_and_dummy_prompt():
    from detikzify_amd.model import DUMMY_IMAGE, AdapterProcessor
    from detikzify_amd.model.tokenizer import SyntheticTokenizer
    from tests.helpers import fake_processor, sketch_image
    inner = fake_processor(512, 12, 84)
    tok = SyntheticTokenizer(300, bos_token_id=1, eos_token_id=2, pad_token_id=0, model_max_length=512)
    proc = AdapterProcessor(processor=inner, tokenizer=tok)
    only_text = proc(text="a red circle", return_tensors="pt")
    assert set(only_text) == {"input_ids", "attention_mask", "adapter_input_ids", "adapter_attention_mask"} - \
        ({"attention_mask"} if "attention_mask" not in inner(images=[DUMMY_IMAGE], return_tensors="pt") else set())
    assert torch.equal(only_text["input_ids"], inner(images=[DUMMY_IMAGE], return_tensors="pt")["input_ids"])
    assert torch.equal(only_text["adapter_input_ids"], torch.tensor([tok.encode("a red circle")]))
    assert bool(only_text["adapter_attention_mask"].all())
    both = proc(text="x" * 600, images=sketch_image(0, 84), text_kwargs={"truncation": True}, return_tensors="pt")
    assert "pixel_values" in both and both["adapter_input_ids"].shape == (1, 512)
    with pytest.raises(ValueError):
        proc()
    from detikzify_amd.util import unwrap_processor
    assert unwrap_processor(proc) is inner


def test_pipeline_refuses_text_without_an_adapter_processor():
    from detikzify_amd.infer import DetikzifyPipeline
    from tests.helpers import fake_processor

    class M:
        adapter = object()
    pipe = object.__new__(DetikzifyPipeline)
    pipe.model, pipe.processor = M(), fake_processor(512, 12, 84)
    with pytest.raises(AssertionError, match="adapter"):
        pipe.check_inputs(None, "a red circle")          # a model with an adapter but the plain processor: the text would be a prompt prefix
