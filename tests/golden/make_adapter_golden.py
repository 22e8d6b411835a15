#!/usr/bin/env python
"""
Generates tests/golden/adapter_tiny.npz from the reference's OWN TikZero adapter module
(detikzify/model/adapter/modeling_adapter.py, loaded in place from the reference checkout given as the first argument):
CrossAttentionAdapter at toy size (D 64, 2 heads of 32, mlp 96, 2 tower layers, cross_attn_every_n_layers 1, eager
attention), fp32, seeded weights with non-zero gates.  Recorded: the adapter's state dict, the connector input (text hidden
states), a tower activation x and every layer's CrossAttentionLayer output on it, and connect(hidden).  Only outputs are
committed; tests/test_adapter_host.py checks tests/adapter_oracle.py against them.  Deterministic.
usage: python tests/golden/make_adapter_golden.py <reference checkout>
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch
from transformers import PretrainedConfig

OUT = Path(__file__).resolve().parent / "adapter_tiny.npz"


def main(ref_root: str):
    spec = importlib.util.spec_from_file_location("ref_modeling_adapter", Path(ref_root) / "detikzify/model/adapter/modeling_adapter.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = PretrainedConfig(hidden_size=64, num_attention_heads=2, intermediate_size=96, layer_norm_eps=1e-6,
                           hidden_act="gelu_pytorch_tanh", attention_dropout=0.0, num_hidden_layers=2, image_size=56,
                           patch_size=14, num_channels=3)
    cfg._attn_implementation = "eager"
    torch.manual_seed(0)
    ad = mod.CrossAttentionAdapter(cfg, input_hidden_size=48, cross_attn_every_n_layers=1).float().eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, p in ad.named_parameters():
            if name.endswith("_gate"):
                p.copy_(torch.tensor([0.7 if "attn_gate" in name else -0.4]))
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif name == "dummy_input":
                p.copy_(1.5 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
        hidden = torch.randn(1, 7, 48, generator=g)
        x = torch.randn(1, 16, 64, generator=g)
        c = ad.connect(hidden)
        outs = {f"out.{i}": layer(hidden_states=x, cross_attention_states=c, cross_attention_mask=None, attention_mask=None)[0][0].numpy()
                for i, layer in enumerate(ad.layers)}
    data = {"adapter." + k: v.detach().numpy().astype(np.float32) for k, v in ad.state_dict().items()}
    data.update({"hidden": hidden[0].numpy(), "x": x[0].numpy(), "connected": c[0].numpy(), **outs})
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
