"""The oracle of kv_format "mxfp8": LlamaOracle with a boundary `kv_from`.  forward() is restated with the rows >= kv_from of every
layer's keys (after RoPE) and values passed through mx_fake_quant(., 32) — MXFP8 in groups of 32 dims of a head's row — at attention
time.  The stored rows stay bf16 (the cache's master copy), so moving the boundary later changes what the next step sees, as on the
device; in one teacher-forced pass every query sees the rows >= kv_from quantised, the row of its own position included."""
from __future__ import annotations

import torch

from oracle.llama import LlamaOracle, apply_rope, attention, linear, mx_fake_quant, rb, rmsnorm

NO_KV8 = 1 << 30


class Kv8LlamaOracle(LlamaOracle):
    kv_from = NO_KV8          # rows [kv_from, ...) are MXFP8 rows; >= the length: the plain oracle

    def _kv_seen(self, x: torch.Tensor) -> torch.Tensor:
        """[KVH, T, hd] rows as attention reads them"""
        f = max(0, min(self.kv_from, x.shape[1]))
        if f >= x.shape[1]:
            return x
        return torch.cat([x[:, :f], mx_fake_quant(x[:, f:], 32)], dim=1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        P = self.precision
        T = x.shape[0]
        start = self.pos
        cos, sin = self.cos[start:start + T], self.sin[start:start + T]
        for i in range(self.L):
            p = f"model.layers.{i}."
            h = rmsnorm(x, self.w[p + "input_layernorm.weight"], self.cfg["rms_eps"], P)
            if self.act_quant:
                h = mx_fake_quant(h, 32)
            q = linear(h, self.w[p + "self_attn.q_proj.weight"], None, P)
            k = linear(h, self.w[p + "self_attn.k_proj.weight"], None, P)
            v = linear(h, self.w[p + "self_attn.v_proj.weight"], None, P)
            q = q.view(T, self.H, self.hd).transpose(0, 1)
            k = k.view(T, self.KVH, self.hd).transpose(0, 1)
            v = v.view(T, self.KVH, self.hd).transpose(0, 1)
            q, k = apply_rope(q, cos, sin, P), apply_rope(k, cos, sin, P)
            self.k[i] = k if self.k[i] is None else torch.cat([self.k[i], k], dim=1)
            self.v[i] = v if self.v[i] is None else torch.cat([self.v[i], v], dim=1)
            a = attention(q, self._kv_seen(self.k[i]), self._kv_seen(self.v[i]), self.scale, causal_offset=start, precision=P)
            a = a.transpose(0, 1).reshape(T, self.d)
            if self.act_quant:
                a = mx_fake_quant(a, 32)
            x = rb(x + linear(a, self.w[p + "self_attn.o_proj.weight"], None, P), P)
            h = rmsnorm(x, self.w[p + "post_attention_layernorm.weight"], self.cfg["rms_eps"], P)
            if self.act_quant:
                h = mx_fake_quant(h, 32)
            g = linear(h, self.w[p + "mlp.gate_proj.weight"], None, P)
            u = linear(h, self.w[p + "mlp.up_proj.weight"], None, P)
            act = rb(rb(torch.nn.functional.silu(g), P) * u, P)
            if self.act_quant:
                act = mx_fake_quant(act, 16)
            x = rb(x + linear(act, self.w[p + "mlp.down_proj.weight"], None, P), P)
        self.pos = start + T
        return x


def kv8_oracle(cfg, weights, precision="bf16", kv_from=NO_KV8):
    """a DetikzifyOracle whose decoder is the kv8 oracle"""
    from oracle.model import DetikzifyOracle
    o = DetikzifyOracle(cfg, weights, precision=precision)
    llm = Kv8LlamaOracle(o.llm.cfg, o.llm.w, o.llm.precision)
    llm.act_quant = o.llm.act_quant
    llm.kv_from = kv_from
    o.llm = llm
    return o
