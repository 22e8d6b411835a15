"""CPU restatement of the TikZero adapter (reference detikzify/model/adapter/modeling_adapter.py) on top of the oracle's ViT and
LLaMA helpers: the embedding model's last_hidden_state, the connector, CrossAttentionLayer, and text-conditioned tower features.
Weights: flat fp32 tensors by the reference's names ("adapter.*", "embedding_model.*", "vision_model.*"), shaped here."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from oracle.llama import LlamaOracle, attention, rmsnorm
from oracle.ops import linear, rb
from oracle.vit import VitOracle, gelu, layernorm


def embedding_weights(acfg: dict, w: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """"embedding_model.*" -> the HF LlamaForCausalLM names LlamaOracle reads, shaped"""
    d, ff, V, hd = acfg["hidden"], acfg["ffn"], acfg["vocab"], acfg["head_dim"]
    kvd = acfg["kv_heads"] * hd
    shapes = {"embed_tokens.weight": (V, d), "norm.weight": (d,), "input_layernorm.weight": (d,), "post_attention_layernorm.weight": (d,),
              "self_attn.q_proj.weight": (d, d), "self_attn.k_proj.weight": (kvd, d), "self_attn.v_proj.weight": (kvd, d),
              "self_attn.o_proj.weight": (d, d), "mlp.gate_proj.weight": (ff, d), "mlp.up_proj.weight": (ff, d),
              "mlp.down_proj.weight": (d, ff)}
    out = {}
    for k, v in w.items():
        if not k.startswith("embedding_model."):
            continue
        n = k[len("embedding_model."):]
        if n.startswith("rope."):
            continue            # LlamaOracle computes the llama3 tables itself: the device's (model.rope_tables) are checked, not reused
        tail = n.split(".", 2)[-1] if n.startswith("layers.") else n
        out["model." + n] = v.reshape(shapes[tail])
    return out


def embed_text(acfg: dict, w: Dict[str, torch.Tensor], ids: torch.Tensor, precision: str = "bf16") -> torch.Tensor:
    """embedding_model(input_ids).last_hidden_state: every row after the final RMSNorm -> [T, d]"""
    lw = embedding_weights(acfg, w)
    o = LlamaOracle({**acfg, "max_positions": acfg["text_max"]}, lw, precision)
    h = o.forward(o.embed(ids))
    return rmsnorm(h, lw["model.norm.weight"], acfg["rms_eps"], precision)


def _gate(g: torch.Tensor, P: str) -> torch.Tensor:
    return rb(torch.sigmoid(g.reshape(1)), P)        # a bf16 parameter's sigmoid is a bf16 tensor


class AdapterOracle:
    def __init__(self, vcfg: dict, acfg: dict, w: Dict[str, torch.Tensor], precision: str = "bf16"):
        self.vcfg, self.acfg, self.w, self.P = vcfg, acfg, w, precision
        self.D, self.H = vcfg["vit_dim"], vcfg["vit_heads"]
        self.hd, self.eps, self.mlp = self.D // self.H, vcfg["vit_ln_eps"], vcfg["vit_mlp"]
        self.vit = VitOracle(vcfg, {k: self._vit_shape(k, v) for k, v in w.items() if k.startswith("vision_model.")}, precision)
        self.present = [(i + 1) % acfg["every_n"] == 0 for i in range(vcfg["vit_depth"])]

    def _vit_shape(self, k, v):
        D, mlp = self.D, self.vcfg["vit_mlp"]
        if k.endswith("qkv.weight"):
            return v.reshape(3 * D, D)
        if k.endswith("proj.weight") and "patch_embed" not in k:
            return v.reshape(D, D)
        if k.endswith("fc1.weight"):
            return v.reshape(mlp, D)
        if k.endswith("fc2.weight"):
            return v.reshape(D, mlp)
        return v

    def _lin(self, x, p, n_out, n_in):
        return linear(x, self.w[p + ".weight"].reshape(n_out, n_in), self.w[p + ".bias"], self.P)

    def _heads_ln(self, x, p):
        T = x.shape[0]
        y = layernorm(x.reshape(T, self.H, self.hd), self.w[p + ".weight"], self.w[p + ".bias"], self.eps, self.P)
        return y.transpose(0, 1)                      # [H, T, hd]

    def text_kv(self, ids: torch.Tensor):
        """connector output and every cross layer's (k_norm(k), v) of one text"""
        P, D, de = self.P, self.D, self.acfg["hidden"]
        return self.cross_kv(self._lin(embed_text(self.acfg, self.w, ids, P), "adapter.connector", D, de))

    def cross_kv(self, c: torch.Tensor):
        """every cross layer's (k_norm(k_proj(c)), v_proj(c)) of connector output c [T, D]"""
        D = self.D
        kv = {}
        for i, on in enumerate(self.present):
            if on:
                p = f"adapter.layers.{i}.cross_attn."
                k = self._heads_ln(self._lin(c, p + "k_proj", D, D), p + "k_norm")
                v = self._lin(c, p + "v_proj", D, D).reshape(-1, self.H, self.hd).transpose(0, 1)
                kv[i] = (k, v)
        return kv

    def cross_layer(self, x, i, kv):
        P, D, p = self.P, self.D, f"adapter.layers.{i}."
        h = layernorm(x, self.w[p + "layer_norm1.weight"], self.w[p + "layer_norm1.bias"], self.eps, P)
        q = self._heads_ln(self._lin(h, p + "cross_attn.q_proj", D, D), p + "cross_attn.q_norm")
        a = attention(q, kv[i][0], kv[i][1], 1.0 / math.sqrt(self.hd), None, P).transpose(0, 1).reshape(-1, D)
        o = self._lin(a, p + "cross_attn.out_proj", D, D)
        x = rb(x + rb(_gate(self.w[p + "cross_attn_attn_gate"], P) * o, P), P)
        h = layernorm(x, self.w[p + "layer_norm2.weight"], self.w[p + "layer_norm2.bias"], self.eps, P)
        h = gelu(self._lin(h, p + "mlp.fc1", self.mlp, D), bool(self.vcfg["vit_gelu_tanh"]), P)
        o = self._lin(h, p + "mlp.fc2", D, self.mlp)
        return rb(x + rb(_gate(self.w[p + "cross_attn_mlp_gate"], P) * o, P), P)

    def dummy_pixels(self) -> torch.Tensor:
        S = self.vcfg["vit_image"]
        return self.w["adapter.dummy_input"].reshape(3, S, S).clamp(-1, 1)

    def features(self, pixels: Optional[torch.Tensor], ids: torch.Tensor) -> torch.Tensor:
        """get_intermediate_layers(n=[feature_layer], norm=True) of the tower with the cross layers hooked in -> [N, D]"""
        kv = self.text_kv(ids)
        x = self.vit.embed(self.dummy_pixels() if pixels is None else pixels)
        for i in range(self.vcfg["vit_feature_layer"] + 1):
            if self.present[i]:
                x = self.cross_layer(x, i, kv)
            x = self.vit.block(x, i)
        return self.vit.final_norm(x)
