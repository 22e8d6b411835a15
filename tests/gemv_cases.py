"""Inputs and the float64 reference of the single-sequence decode GEMV op tests (tests/test_gemv_host.py checks them on the CPU,
tests/test_gpu_gemv.py feeds the same objects to dtk_op_gemv_role).

A case holds the operands of ONE role of k_gemv (csrc/kernels_decode.hip): a prologue (COPY, RMSNORM, ATTN), an epilogue (STORE, RESID,
QKV, SWIGLU, LOGITS), a weight format (bf16; fp8 = e4m3 codes x a per-row power-of-two scale; mxfp4 = tests/mxfp4_ref.py's codes and
block scales), a shape and a position.  It is run once per variant of TABLE[(pro, epi, fmt)], the mirror of launch_gemv_variant /
launch_gemv_f8_variant / launch_gemv_q4 kept below as (R, U, waves, blocks per CU of a persistent grid or 0, KS).

Reference: the dot products in float64 over the exact operand values, rounded to bf16, then gemv_epilogue's rounding chain with
oracle/llama.py's rmsnorm / apply_rope and the oracle's SwiGLU / residual lines.  mode="f32" is the same chain on oracle.ops.linear:
the second legitimate reference, whose distance from the first sets the bar of the chained outputs.  PRO_ATTN: x = sum_s e^(m_s - M) o_s
/ sum_s e^(m_s - M) l_s in float64 (float32 in mode "f32"), rounded to bf16 once.

Operands.  Random cases: x ~ N(0, 1), rows of one magnitude K^-1/2; fp8 rows carry the scales 2^(b + r % 7) over codes sized inversely
(seven binades: neighbours, rows 16 / 64 apart, the RoPE partners hd/2 apart and the gate / up partners ff apart all differ, so one
row's scale on another is a factor >= 2); mxfp4 rows alternate the magnitude of their 32-blocks by (block + row) % 2, so neighbouring
blocks carry different scales.  GRID cases: x and W on a grid of eighths (mxfp4: E2M1 values x 2^{-1, 0, 1}), so every fp32 partial
sum is exact in any order and the projection has ONE value: what they write must equal the reference bit for bit.  Under PRO_RMSNORM a
GRID x is +-1 (mean square 1: x * rsqrt(1 + eps) rounds to +-1 in bf16 whatever the last bits of the rsqrt) and norm_w is on the grid;
under PRO_ATTN all maxima are equal (weights e^0 = 1, and e^(-1e30 - M) = 0 for the empty split), the l sum to a power of two and the o
are eighths: the input is exact again.  Only the SwiGLU activation (expf) keeps the chained bar on GRID operands.
pos: T_MAX - 1 and the interior POS_IN, never 0 (sin = 0 would hide a RoPE sign).  PRO_ATTN partials: m within a few units of 0,
l > 0, the last but one split empty exactly as the attention kernels leave it (m = -1e30, l = 0, o = 0) where S >= 3.

Every result buffer starts as a quiet NaN with a payload of its own (the residual excepted: it is an input); judge() demands that every
cell outside the ones the role writes still holds its bits.

Bars.  Single-rounding outputs (PRO_COPY: STORE, the RESID projection = result - residual in float64): test_op_gemv's rel-L2 < 1e-3,
<= 2.01 bf16 ulps, < 5 % of the elements differing.  Chained outputs (everything downstream of PRO_RMSNORM / PRO_ATTN, q / k after RoPE
in ulps of the pair's length, SwiGLU, the residual after the add): twice the worst distance between the two references over every case
of this file and nine more operand draws of its small ones (redraws(): the two references differ by a rounding flip about once in
10^4 outputs, so the case list alone is too small a sample), capped at test_op_attention's 4.01 ulps / 2e-3.  Measured (tests/
test_gemv_host.py asserts the figures): 4.96 ulps (V rows of hd-64 q/k/v at K = 72 beside zero, where the 1 % floor of ulp_report
counts a change of 1e-3 of a typical element as several ulps) and rel-L2 2.53e-3 (the same 384 values; SwiGLU at ff = 8 1.5e-3): both
beyond the caps, so the bar IS the caps.

Unreachable at any shape the entry point admits (so not exercised): the clamped unit tail (u >= n_units) of EPI_QKV outside the
persistent shapes — a head is 32 or 64 units and no block owns more than 16, so the units are a multiple of every R x waves — and of
EPI_SWIGLU for R x waves <= 8 (ff % 8 == 0)."""
from __future__ import annotations

import os

import numpy as np
import torch

from oracle.llama import apply_rope, rmsnorm, rope_tables
from oracle.ops import bits_to_f32, f32_to_bits, linear, rb
from tests import mxfp4_ref
from tests.gemv_b_cases import ulp_report

COPY, RMSNORM, ATTN = 0, 1, 2
STORE, RESID, QKV, SWIGLU, LOGITS = 0, 1, 2, 3, 4
PRO_NAME = {COPY: "copy", RMSNORM: "norm", ATTN: "attn"}
EPI_NAME = {STORE: "store", RESID: "resid", QKV: "qkv", SWIGLU: "swiglu", LOGITS: "logits"}
T_MAX, POS_IN = 8, 3
EPS = 1e-5
NAN_Q, NAN_K, NAN_V, NAN_Y, NAN_LOGITS = 0x7FC1, 0x7FC2, 0x7FC3, 0x7FC4, 0x7FC00007       # quiet NaNs, one payload per buffer

SINGLE_RL2, SINGLE_ULPS, SINGLE_FRAC = 1e-3, 2.01, 0.05                 # test_op_gemv
MEASURED_CHAIN_ULPS, MEASURED_CHAIN_RL2 = 4.96, 2.53e-3                 # float64 vs float32 reference, worst over every case below and its redraws
CHAIN_ULPS, CHAIN_RL2 = min(4.01, 2 * MEASURED_CHAIN_ULPS), min(2e-3, 2 * MEASURED_CHAIN_RL2)

MUTATIONS = ("pos_off", "rope_sign", "rope_partner_scale", "gate_up_swap", "kv_section_shift", "drop_kgroup", "dup_kgroup", "drop_tail_chunk",
             "scale_up", "scale_down", "resid_once", "attn_split_dropped", "attn_unnormalised", "f4_block_shift")

# ---------------------------------------------------------------------------------------------------- the launchers' tables
# variant -> (R, U, waves, blocks per CU of the persistent grid | 0 = one chunk per wave, KS)
_PAIRED = {0: (1, 2, 4, 0, 1), 8: (2, 2, 4, 0, 1), 9: (1, 1, 4, 0, 1), 10: (1, 2, 8, 0, 1), 11: (1, 2, 2, 0, 1), 1: (1, 4, 4, 0, 1), 2: (2, 2, 8, 0, 1),
           3: (2, 2, 4, 4, 1), 4: (2, 2, 8, 2, 1), 5: (1, 4, 8, 2, 1), 6: (4, 1, 4, 0, 1), 7: (1, 2, 4, 0, 1)}
_F8_PAIRED = {1: (2, 2, 4, 0, 1), 0: (1, 2, 4, 0, 1), 2: (2, 4, 4, 0, 1), 3: (4, 2, 4, 0, 1), 4: (2, 2, 8, 0, 1), 5: (1, 4, 4, 0, 1), 6: (1, 2, 4, 4, 1),
              7: (2, 2, 4, 4, 1), 8: (1, 2, 8, 2, 1), 9: (1, 4, 4, 4, 1)}
TABLE = {
    (RMSNORM, QKV, "bf16"): _PAIRED,
    (RMSNORM, SWIGLU, "bf16"): _PAIRED,
    (COPY, RESID, "bf16"): {0: (1, 8, 4, 0, 1), 8: (2, 4, 4, 0, 1), 9: (1, 2, 4, 0, 1), 10: (1, 8, 8, 0, 1), 11: (1, 8, 2, 0, 1), 12: (1, 4, 2, 0, 1),
                            1: (1, 4, 4, 0, 1), 2: (4, 2, 4, 0, 1), 3: (2, 4, 8, 0, 1), 4: (2, 4, 4, 4, 1), 5: (2, 4, 8, 2, 1), 6: (1, 8, 4, 0, 1),
                            7: (2, 2, 4, 0, 1), 13: (1, 4, 8, 0, 2), 14: (2, 4, 8, 0, 2), 15: (1, 6, 8, 0, 2), 16: (2, 6, 8, 0, 2), 17: (1, 6, 16, 0, 4),
                            18: (1, 2, 16, 0, 4), 19: (1, 3, 8, 0, 2), 20: (1, 4, 4, 0, 2), 21: (1, 6, 4, 0, 2), 22: (4, 2, 8, 0, 2)},
    (ATTN, RESID, "bf16"): {0: (2, 4, 8, 0, 1), 1: (2, 4, 4, 0, 1), 2: (1, 8, 8, 0, 1), 3: (4, 2, 8, 0, 1), 4: (4, 2, 4, 0, 1), 5: (2, 4, 8, 0, 2),
                            6: (4, 4, 8, 0, 2), 7: (2, 4, 16, 0, 1), 8: (2, 4, 16, 0, 2)},
    (RMSNORM, LOGITS, "bf16"): {0: (2, 4, 4, 0, 1), 1: (4, 2, 8, 2, 1), 2: (4, 2, 4, 0, 1), 3: (1, 4, 4, 0, 1), 4: (1, 8, 4, 0, 1)},
    (RMSNORM, STORE, "bf16"): {0: (4, 2, 4, 0, 1), 20: (1, 2, 4, 0, 1)},
    (COPY, STORE, "bf16"): {0: (4, 2, 4, 0, 1), 20: (1, 2, 4, 0, 1), 21: (1, 8, 4, 0, 1)},
    (RMSNORM, QKV, "fp8"): _F8_PAIRED,
    (RMSNORM, SWIGLU, "fp8"): _F8_PAIRED,
    (RMSNORM, LOGITS, "fp8"): {**{v: (4, 2, 4, 0, 1) for v in (1, 4, 5, 6, 7, 8, 9)}, 0: (2, 2, 4, 0, 1), 2: (4, 4, 4, 0, 1), 3: (8, 2, 4, 0, 1)},
    (ATTN, RESID, "fp8"): {v: (2, 2, 4, 0, 1) for v in range(10)},
    (COPY, RESID, "fp8"): {1: (2, 4, 4, 0, 1), 0: (1, 4, 4, 0, 1), 2: (2, 8, 4, 0, 1), 3: (4, 4, 4, 0, 1), 4: (2, 4, 8, 0, 1), 5: (1, 8, 4, 0, 1),
                           6: (1, 4, 4, 4, 1), 7: (2, 4, 4, 4, 1), 8: (1, 4, 8, 2, 1), 9: (1, 8, 4, 4, 1)},
    (RMSNORM, QKV, "mxfp4"): {-1: (1, 2, 8, 2, 1)},
    (RMSNORM, SWIGLU, "mxfp4"): {-1: (1, 2, 8, 2, 1)},
    (ATTN, RESID, "mxfp4"): {-1: (2, 2, 4, 0, 1)},
    (COPY, RESID, "mxfp4"): {-1: (2, 2, 4, 0, 1)},
    (RMSNORM, STORE, "mxfp4"): {-1: (2, 2, 4, 0, 1)},
    (COPY, STORE, "mxfp4"): {-1: (2, 2, 4, 0, 1)},
}
ELEMS_PER_CHUNK = {"bf16": 8, "fp8": 16, "mxfp4": 32}          # weights in a 16-byte chunk of a row


def f8_default():
    return int(os.environ.get("DTK_F8_VARIANT", "8"))


def default_variant(pro, epi, fmt, K, d):
    """what variant -1 runs (launch_gemv with nothing chosen by dtk_set_gemv_variant)"""
    if fmt == "mxfp4":
        return -1
    if fmt == "fp8":
        return f8_default()
    if pro == ATTN:
        return 8 if d > 2048 else 1
    o_proj = epi == RESID and K == d
    if 0 < d <= 2048:
        return {SWIGLU: 5, RESID: 1 if o_proj else 15, LOGITS: 3}.get(epi, 0)
    if d > 2048:
        return {RESID: 10, LOGITS: 3}.get(epi, 0)
    return 0


def chunks(fmt, K):
    """16-byte chunks of one weight row (KC of k_gemv)"""
    e = ELEMS_PER_CHUNK[fmt]
    return (K + e - 1) // e


def groups(fmt, K, U, KS=1):
    """k-groups of each of the KS waves that share a row (G of k_gemv): [G_0, .., G_KS-1]"""
    gall = -(-(-(-chunks(fmt, K) // 64)) // U)
    return [(gall - ks + KS - 1) // KS for ks in range(KS)]


def has_full_group(fmt, K, U):
    return chunks(fmt, K) >= 64 * U


def has_ragged_group(fmt, K, U):
    return chunks(fmt, K) % (64 * U) != 0


def rope_pair_magnitude(o, hd):
    """o [heads * hd] after RoPE -> the length of each (i, i + hd/2) pair at both of its places: o1 = x1 c - x2 s can be far smaller than
    its terms, and one legitimate rounding flip of x1 is then many ulps OF o1; what a flip moves is bounded in ulps of the pair's length"""
    t = o.reshape(-1, 2, hd // 2)
    return t.pow(2).sum(1, keepdim=True).sqrt().expand_as(t).reshape(-1)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


class Case:
    def __init__(self, pro, epi, fmt, K=0, N=0, H=0, KVH=0, hd=128, ff=0, S=0, grid=False, pos=T_MAX - 1, seed=0, tag=""):
        self.pro, self.epi, self.fmt, self.grid, self.pos, self.tag = pro, epi, fmt, grid, pos, tag
        self.H, self.KVH, self.hd, self.ff, self.S = H, KVH, hd, ff, S
        if pro == ATTN:
            K = H * hd
        self.K = K
        self.N = N if epi in (STORE, RESID, LOGITS) else ((H + 2 * KVH) * hd if epi == QKV else 2 * ff)
        self.units = self.N // 2 if epi in (QKV, SWIGLU) else self.N
        self.d = H * hd if epi == QKV else 0
        N = self.N
        g = torch.Generator().manual_seed(100003 * pro + 1009 * epi + 7 * K + 31 * N + {"bf16": 0, "fp8": 500, "mxfp4": 900}[fmt] + 13 * S + hd + seed)
        self.norm_w = None
        self.W8 = self.W4 = self.S4 = self.wscale = None
        # ---- the input vector
        if pro == ATTN:
            self._partials(g)
        elif grid and pro == RMSNORM:
            self.x = (torch.randint(0, 2, (K,), generator=g) * 2 - 1).float()
            self.norm_w = torch.randint(-16, 17, (K,), generator=g).float() / 8
        elif grid:
            self.x = torch.randint(-8, 9, (K,), generator=g).float() / 8
        else:
            self.x = rb(torch.randn(K, generator=g))
        if pro == RMSNORM and not grid:
            self.norm_w = rb(1 + 0.1 * torch.randn(K, generator=g))
        # ---- the weights
        e = torch.arange(N) % 7
        if fmt == "mxfp4":
            KC = (K + 31) // 32
            if grid:
                e2m1 = torch.tensor(np.concatenate([mxfp4_ref.GRID, -mxfp4_ref.GRID]), dtype=torch.float32)
                eb = torch.randint(-1, 2, (N, KC), generator=g).float()
                W = e2m1[torch.randint(0, 16, (N, KC * 32), generator=g)] * torch.exp2(eb).repeat_interleave(32, 1)
                W[:, ::32] = 6 * torch.exp2(eb) * (torch.randint(0, 2, (N, KC), generator=g) * 2 - 1)        # pins the block scale
                W = W[:, :K]
            else:
                blk = (torch.arange(K)[None, :] // 32 + torch.arange(N)[:, None]) % 2
                W = rb(torch.randn(N, K, generator=g) * K ** -0.5 * torch.exp2(blk.float()))
            self.W4, self.S4, weff = mxfp4_ref.quantise(W.numpy())
            self.W = torch.from_numpy(mxfp4_ref.dequantise(self.W4, self.S4, K)).float()
            assert np.array_equal(self.W.double().numpy(), weff) and (not grid or torch.equal(self.W, W))
        elif fmt == "fp8":
            if grid:
                q = torch.randint(-8, 9, (N, K), generator=g).float()
                self.wscale = torch.exp2(-3.0 - e)
            else:     # codes of magnitude ~ 8 * 2^-(r % 7) under the scale 2^(b + r % 7): de-quantised rows of one magnitude, ~ K^-1/2
                q = (torch.randn(N, K, generator=g) * 8 * torch.exp2(-e.float())[:, None]).to(torch.float8_e4m3fn).float()
                self.wscale = torch.exp2(-3.0 - round(0.5 * float(np.log2(K))) + e)
            self.W8 = q.to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()
            assert torch.equal(torch.from_numpy(self.W8).view(torch.float8_e4m3fn).float(), q)
            self.Wq = q
            self.W = q * self.wscale[:, None]
            for gap in (1, 16, 64, hd // 2) + ((ff,) if epi == SWIGLU else ()):
                assert gap >= N or bool((e[gap:] != e[:-gap]).all()), (self.name, gap)
        else:
            self.W = torch.randint(-8, 9, (N, K), generator=g).float() / 8 if grid else rb(torch.randn(N, K, generator=g) * K ** -0.5)
        assert torch.equal(rb(self.W), self.W)
        # ---- the role's other operands
        self._ref = {}
        self.res = None
        if epi == RESID:
            if grid:
                self.res = rb(torch.randn(N, generator=g))
            else:
                # The bar of the RESID projection is a single rounding's, and result - residual gives the projection back only if the add
                # rounds nothing away: the residual is -sign(p) * m ulps of the reference projection, m = 1..3, so residual + bf16(p) is a
                # bf16 number for the reference's p and for a p one ulp beside it.  (What the add rounds is the GRID cases' matter.)
                p = rb((self.x_in().double() @ self.W.double().t()).float())
                ulp = torch.exp2(torch.floor(torch.log2(p.abs().clamp(min=2.0 ** -20))) - 7)
                m = torch.randint(1, 4, p.shape, generator=g).float()
                self.res = -torch.sign(p + (p == 0)) * m * ulp
                assert torch.equal(rb(self.res), self.res) and torch.equal(rb(self.res + p), self.res + p)
        if epi == QKV:
            self.cos, self.sin = rope_tables(hd, 10000.0, 1.0, T_MAX)

    def _partials(self, g):
        H, S, hd = self.H, self.S, self.hd
        if self.grid:
            self.pm = torch.full((H, S), 0.75)
            ls = {1: [2.0], 3: [1.0, 1.0, 2.0], 4: [1.0] * 4, 5: [1.0, 1.0, 2.0, 2.0, 2.0], 16: [1.0] * 16}[S]
            self.pl = torch.tensor(ls).repeat(H, 1)
            self.po = torch.randint(-8, 9, (H, S, hd), generator=g).float() / 8
        else:
            self.pm = torch.randn(H, S, generator=g) * 2
            self.pl = 0.5 + 3.5 * torch.rand(H, S, generator=g)
            self.po = torch.randn(H, S, hd, generator=g) * self.pl[:, :, None]
        if S >= 3:        # an empty split, as k_attn_decode leaves it
            self.pm[:, S - 2], self.pl[:, S - 2], self.po[:, S - 2] = -1e30, 0.0, 0.0
            if self.grid:
                self.pl[:, 0] += {3: 1.0, 4: 1.0, 5: 2.0, 16: 1.0}[S]         # (the sum stays a power of two)

    def combine(self, mode="f64", mutate=None):
        """the PRO_ATTN input [K]: the flash-decode reduction of the partials, rounded to bf16 once"""
        dt = torch.float64 if mode == "f64" else torch.float32
        m, l, o = self.pm.to(dt), self.pl.to(dt), self.po.to(dt)
        w = torch.exp(m - m.max(1, keepdim=True)[0])
        if mutate == "attn_split_dropped":
            w = w.clone(); w[:, self.S - 1] = 0
        L = (w * l).sum(1, keepdim=True)
        x = (w[:, :, None] * o).sum(1)
        if mutate != "attn_unnormalised":
            x = x / L
        return rb(x.float()).reshape(-1)

    def x_in(self, mode="f64", mutate=None):
        """the GEMV's input vector: x, its RMSNorm, or the combine of the partials"""
        if self.pro == ATTN:
            return self.combine(mode, mutate)
        if self.pro != RMSNORM:
            return self.x
        if mode == "f32":
            return rmsnorm(self.x, self.norm_w, EPS)
        x = self.x.double()         # oracle/llama.py's rmsnorm with the mean square and its rsqrt in float64: the same two rounding points
        return rb(self.norm_w * rb((x * torch.rsqrt(x.pow(2).mean() + EPS)).float()))

    @property
    def name(self):
        shape = {QKV: f"H{self.H}KVH{self.KVH}hd{self.hd}-pos{self.pos}", SWIGLU: f"ff{self.ff}"}.get(self.epi, f"N{self.N}")
        if self.pro == ATTN:
            shape += f"-H{self.H}hd{self.hd}S{self.S}"
        return f"{PRO_NAME[self.pro]}-{EPI_NAME[self.epi]}-{shape}-K{self.K}-{self.fmt}" + ("-grid" if self.grid else "") + self.tag

    @property
    def chained(self):
        return self.pro != COPY

    def variants(self):
        return sorted(TABLE[(self.pro, self.epi, self.fmt)])

    # ------------------------------------------------------------------ reference
    def applies(self, m):
        wide = self.units >= 16          # a statistical fault (a fraction of a sum lost) needs more than a handful of outputs to show for certain
        return {"pos_off": self.epi == QKV, "rope_sign": self.epi == QKV, "rope_partner_scale": self.epi == QKV and self.fmt == "fp8",
                "gate_up_swap": self.epi == SWIGLU, "kv_section_shift": self.epi == QKV and self.KVH < self.H,
                "drop_kgroup": wide, "dup_kgroup": wide, "drop_tail_chunk": wide and self.K % 512 != 0,
                "scale_up": wide and self.fmt == "fp8", "scale_down": wide and self.fmt == "fp8",
                "resid_once": self.grid and self.epi == RESID and self.N >= 100 and self.K >= 64,      # (8 products of eighths are a bf16 number: nothing to round twice)
                "attn_split_dropped": self.pro == ATTN and self.S > 1, "attn_unnormalised": self.pro == ATTN,
                "f4_block_shift": wide and self.fmt == "mxfp4" and self.K > 32}[m]

    def reference(self, mode="f64", mutate=None):
        """the role's outputs (fp32 tensors of bf16 values): p (the rounded projection) and, per role, y / act / q, k, v; pos = the cache
        row written"""
        if mutate is None and mode in self._ref:
            return self._ref[mode]
        xin = self.x_in(mode, mutate)
        W, pos, K = self.W, self.pos, self.K
        span = min(K, 512)                      # the wave-load of bf16 chunks the wrong references lose or repeat
        lo = (K // span) // 2 * span
        if mutate == "drop_kgroup":
            xin = xin.clone(); xin[lo:lo + span] = 0
        elif mutate == "drop_tail_chunk":
            xin = xin.clone(); xin[K - 8:] = 0
        elif mutate in ("scale_up", "scale_down"):
            W = self.Wq * torch.roll(self.wscale, 1 if mutate == "scale_down" else -1)[:, None]      # row r with the scale of row r -+ 1
        elif mutate == "f4_block_shift":
            W = torch.from_numpy(mxfp4_ref.dequantise(self.W4, np.roll(self.S4, 1, axis=1), K)).float()
        elif mutate == "pos_off":
            pos = pos + 1 if pos < T_MAX - 1 else pos - 1
        if mode == "f64":
            acc = xin.double() @ W.double().t()
            if mutate == "dup_kgroup":
                acc = acc + xin[lo:lo + span].double() @ W[:, lo:lo + span].double().t()
            p = rb(acc.float())
        else:
            assert mutate is None
            acc = None
            p = linear(xin[None, :], W)[0]
        out = {"p": p, "pos": pos}
        if self.epi == QKV:
            H, KVH, hd = self.H, self.KVH, self.hd
            if mutate == "rope_partner_scale":      # the scale of r0 on r0 + hd/2
                t = acc.float().reshape(-1, 2, hd // 2) / self.wscale.reshape(-1, 2, hd // 2)
                p = rb((t * self.wscale.reshape(-1, 2, hd // 2)[:, :1]).reshape(-1))
            heads = p.reshape(H + 2 * KVH, 1, hd)
            nk = KVH - 1 if mutate == "kv_section_shift" else KVH      # the last k head taken for the first v head
            cos, sin = self.cos[pos][None, :], self.sin[pos][None, :]
            if mutate == "rope_sign":
                sin = -sin
            out["q"] = apply_rope(heads[:H], cos, sin).reshape(H, hd)
            out["k"] = apply_rope(heads[H:H + nk], cos, sin).reshape(nk, hd)
            out["v"] = heads[H + nk:H + nk + KVH].reshape(KVH, hd)
        elif self.epi == SWIGLU:
            gate, up = p[:self.ff], p[self.ff:]
            if mutate == "gate_up_swap":
                gate, up = up, gate
            out["act"] = rb(rb(torch.nn.functional.silu(gate)) * up)
        elif self.epi == RESID:
            out["y"] = rb(self.res + (acc.float() if mutate == "resid_once" else p))
        if mutate is None:
            self._ref[mode] = out
        return out

    # ------------------------------------------------------------------ buffers
    def initial(self):
        """the in/out buffers before the run (numpy bit patterns)"""
        if self.epi == QKV:
            kv = (self.KVH, T_MAX, self.hd)
            return {"q": np.full(self.H * self.hd, NAN_Q, dtype=np.uint16), "k": np.full(kv, NAN_K, dtype=np.uint16), "v": np.full(kv, NAN_V, dtype=np.uint16)}
        if self.epi == LOGITS:
            return {"logits": np.full(self.N, NAN_LOGITS, dtype=np.uint32).view(np.float32)}
        if self.epi == RESID:
            return {"y": f32_to_bits(self.res)}
        return {"y": np.full(self.ff if self.epi == SWIGLU else self.N, NAN_Y, dtype=np.uint16)}

    def written(self, out):
        """what a run that computes `out` leaves in the buffers"""
        buf = self.initial()
        if self.epi == QKV:
            buf["q"][:] = f32_to_bits(out["q"]).reshape(-1)
            buf["k"][:out["k"].shape[0], out["pos"]] = f32_to_bits(out["k"])
            buf["v"][:, out["pos"]] = f32_to_bits(out["v"])
        elif self.epi == LOGITS:
            buf["logits"][:] = out["p"].numpy()
        else:
            buf["y"][:] = f32_to_bits(out[{SWIGLU: "act", RESID: "y", STORE: "p"}[self.epi]])
        return buf

    def write_mask(self):
        """True where the role writes"""
        ref = self.reference()
        a, b = (self.written({k: (torch.full_like(v, c) if torch.is_tensor(v) else v) for k, v in ref.items()}) for c in (1.0, 2.0))
        return {n: _bits(a[n]) != _bits(b[n]) for n in a}

    def extract(self, got):
        f = lambda bits: bits_to_f32(np.ascontiguousarray(bits)).reshape(-1)
        if self.epi == QKV:
            return {"q": f(got["q"]), "k": f(got["k"][:, self.pos]), "v": f(got["v"][:, self.pos])}
        if self.epi == LOGITS:
            return {"p": torch.from_numpy(got["logits"].copy())}
        return {{SWIGLU: "act", RESID: "y", STORE: "p"}[self.epi]: f(got["y"])}

    def pairs(self, out):
        """(single-rounding pairs, chained pairs) of (got, reference[, magnitude]) flat tensors"""
        ref = self.reference()
        flat = lambda t: t.reshape(-1)
        if self.epi == QKV:      # (always behind PRO_RMSNORM: V is chained too)
            rq, rk = flat(ref["q"]), flat(ref["k"])
            if self.grid:
                return [], [(out["v"], flat(ref["v"])), (out["q"], rq), (out["k"], rk)]
            return [], [(out["v"], flat(ref["v"])), (out["q"], rq, rope_pair_magnitude(rq, self.hd)), (out["k"], rk, rope_pair_magnitude(rk, self.hd))]
        if self.epi == SWIGLU:
            return [], [(out["act"], ref["act"])]
        if self.epi in (LOGITS, STORE):
            pr = [(out["p"], ref["p"])]
            return ([], pr) if self.chained else (pr, [])
        chain = [(out["y"], ref["y"])]
        proj = [] if self.grid else [((out["y"].double() - self.res.double()).float(), ref["p"])]   # (a GRID residual is as large as the projection: held to equality instead)
        return ([], chain + proj) if self.chained else (proj, chain)

    def reference_distance(self):
        """worst (ulps, rel-L2) of the chained outputs between the float32 and the float64 reference"""
        far = self.reference("f32")
        out = {k: (v.reshape(-1) if torch.is_tensor(v) else v) for k, v in far.items()}
        wu = wr = 0.0
        for c_ in self.pairs(out)[1]:
            _, u, r = ulp_report(*c_)
            wu, wr = max(wu, u), max(wr, r)
        return wu, wr

    def judge(self, got):
        """got = the buffers after the run.  Returns (ok, figures): cells outside the role's own bit-equal to what they held, single-rounding
        and chained outputs under their bars; GRID cases: every written cell equal to the reference's bit for bit (SwiGLU excepted)"""
        ref = self.reference()
        want, init, mask = self.written(ref), self.initial(), self.write_mask()
        fig = {"untouched": True, "exact": True, "single": (0.0, 0.0, 0.0), "chain": (0.0, 0.0)}
        for name in want:
            g8, i8, w8 = _bits(got[name]), _bits(init[name]), _bits(want[name])
            if not np.array_equal(g8[~mask[name]], i8[~mask[name]]):
                fig["untouched"] = False
            if self.grid and self.epi != SWIGLU and not np.array_equal(g8[mask[name]], w8[mask[name]]):
                fig["exact"] = False
        single, chain = self.pairs(self.extract(got))
        worse = lambda x, y: float("nan") if (x != x or y != y) else max(x, y)
        for a, b in single:
            fig["single"] = tuple(worse(x, y) for x, y in zip(fig["single"], ulp_report(a, b)))
        for c_ in chain:
            fig["chain"] = tuple(worse(x, y) for x, y in zip(fig["chain"], ulp_report(*c_)[1:]))
        fr, u, r = fig["single"]
        cu, cr = fig["chain"]
        ok = fig["untouched"] and fig["exact"] and fr < SINGLE_FRAC and u <= SINGLE_ULPS and r < SINGLE_RL2 and cu <= CHAIN_ULPS and cr < CHAIN_RL2
        return bool(ok), fig


# ---------------------------------------------------------------------------------------------------- the case lists
_cache = {}


def _case(*a, **kw):
    key = (a, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = Case(*a, **kw)
        _cache[key].ctor = (a, kw)
    return _cache[key]


DISTANCE_DRAWS = 10


def redraws(case):
    """the case on other operand draws (seeds 1 ..): not run anywhere, they only widen the sample the distance between the two
    references is taken over.  Two legitimate orders differ by a rounding flip about once in 10^4 outputs, and the bar has to hold one:
    the case list alone has too few outputs for its worst distance to contain a flip reliably."""
    if not case.chained or case.grid or case.N * case.K > 5e5 or not hasattr(case, "ctor"):      # (the small tensors, where one flip weighs most)
        return []
    a, kw = case.ctor
    return [Case(*a, **{**kw, "seed": kw.get("seed", 0) + 1000 * s}) for s in range(1, DISTANCE_DRAWS)]


# K: one ragged chunk; a full wave-load + a 1-lane tail (bf16 520, fp8 1040, mxfp4 2056); both sides of the norm paths' K8 <= 2 * THREADS
# (2048 | 2056, 4096 | 4104, 8200); 1 / 2 / >= 3 k-groups at every U (12296: five groups of 6 wave-loads, dealt 2 1 1 1 over split-K 4; 24584: nine, so that a wave of split-K 4 holds three;
# fp8 16400: three groups of 8)
K_BF16 = (8, 72, 520, 1032, 2048, 2056, 4096, 4104, 8200, 11008)
K_FP8 = (16, 1040, 2048, 4096, 4112, 8208, 11008)
K_OF = {"bf16": K_BF16, "fp8": K_FP8, "mxfp4": K_BF16}
N_TAILS = (1, 37, 130, 257)            # below one block; not a multiple of R, or of R x waves
FF = (8, 24, 88)
HEADS = ((2, 2), (2, 1), (4, 1))
ATTN_S = (1, 3, 4, 5, 16)


def _tails(i, K):
    """two of the four N tails per K, every tail at several K; a call stays under 4 MB of bf16 weights"""
    a, b = ((1, 130), (37, 257))[i % 2]
    return (a, b if b * K * 2 < 4e6 else 130 if 130 * K * 2 < 4e6 else 37)


def proj_cases(pro, epi, fmt):
    """STORE / RESID / LOGITS over the K list x the N tails; GRID operands at K = 72 (8: one chunk), 2056 and 8200 on the larger tails"""
    ks = K_OF[fmt] + (((12296, 24584) if fmt == "bf16" else (16400,) if fmt == "fp8" else ()) if (pro, epi) == (COPY, RESID) else ())
    out = []
    for i, K in enumerate(ks):
        out += [_case(pro, epi, fmt, K, N=n) for n in _tails(i, K)]
    gk = {"bf16": (8, 72, 2056, 8200), "fp8": (16, 1040, 4112, 8208), "mxfp4": (8, 72, 2056, 8200)}[fmt]
    return list(dict.fromkeys(out)) + [_case(pro, epi, fmt, K, N=n, grid=True) for K, n in zip(gk, (130, 257, 257, 130))]


def swiglu_cases(fmt):
    ks = K_OF[fmt]
    out = []
    for i, K in enumerate(ks):
        # (mxfp4, K 11008, ff 24 at seed 0: the two references differ by one flip of a gate, 2.04e-3 of these 24 values — past the cap)
        out += [_case(RMSNORM, SWIGLU, fmt, K, ff=f, seed=int((fmt, K) == ("mxfp4", 11008))) for f in ((FF[i % 3], FF[(i + 1) % 3]) if K < 8000 else (FF[i % 2],))]
    gk = {"bf16": (72, 2056), "fp8": (1040, 4112), "mxfp4": (72, 2056)}[fmt]
    return out + [_case(RMSNORM, SWIGLU, fmt, K, ff=88, grid=True) for K in gk]


def qkv_cases(fmt):
    """(H, KVH) x hd 128 / 64: all six at the two smallest K; above, two per K in turn (N x K stays small), both positions in turn; the
    largest K (the 8-wave shapes' two-pass norm) on the smallest shape only"""
    ks = [K for K in K_OF[fmt] if K <= 8208]
    shapes = [(h, kvh, hd) for hd in (128, 64) for h, kvh in HEADS]
    out, j = [], 0
    for i, K in enumerate(ks):
        if i < 2:
            pick = shapes
        elif K >= 8000:
            pick = [(2, 1, 64)]
        else:
            pick = [shapes[j % 6], shapes[(j + 3) % 6]]
            j += 1
        for n, (h, kvh, hd) in enumerate(pick):
            out.append(_case(RMSNORM, QKV, fmt, K, H=h, KVH=kvh, hd=hd, pos=(T_MAX - 1, POS_IN)[(i + n) % 2]))
    gk = {"bf16": (72, 2056), "fp8": (1040, 4112), "mxfp4": (72, 2056)}[fmt]
    for K, pos in zip(gk, (POS_IN, T_MAX - 1)):
        out += [_case(RMSNORM, QKV, fmt, K, H=h, KVH=kvh, hd=hd, pos=pos, grid=True) for h, kvh, hd in shapes]
    return out


def attn_cases(fmt):
    """S x H at hd 128 (H 2, 4; 10, 20, 33, 65: K = 1280 .. 8320, so that the k-loop turns over at every U) and hd 64 (H 4, 8, 66),
    random weights with N 37 / 256"""
    out = []
    for i, (H, hd) in enumerate(((2, 128), (4, 128), (4, 64), (8, 64), (10, 128), (20, 128), (33, 128), (65, 128), (66, 64))):
        for j in range(2 if H <= 8 else 1):
            S = ATTN_S[(2 * i + j) % 5]
            out.append(_case(ATTN, RESID, fmt, H=H, hd=hd, S=S, N=(37, 256)[(i + j) % 2] if H < 60 else 37))
    out += [_case(ATTN, RESID, fmt, H=4, hd=128, S=16, N=37), _case(ATTN, RESID, fmt, H=8, hd=64, S=1, N=256)]
    out += [_case(ATTN, RESID, fmt, H=H, hd=hd, S=S, N=130, grid=True) for H, hd, S in ((2, 128, 3), (8, 64, 5), (4, 128, 16), (4, 64, 1), (20, 128, 4))]
    return list(dict.fromkeys(out))


ROLES = [(pro, epi, fmt) for fmt in ("bf16", "fp8", "mxfp4") for pro, epi in ((COPY, STORE), (RMSNORM, STORE), (COPY, RESID), (ATTN, RESID),
                                                                             (RMSNORM, QKV), (RMSNORM, SWIGLU), (RMSNORM, LOGITS))
         if (pro, epi, fmt) in TABLE]


def role_cases(pro, epi, fmt):
    if pro == ATTN:
        return attn_cases(fmt)
    if epi == QKV:
        return qkv_cases(fmt)
    if epi == SWIGLU:
        return swiglu_cases(fmt)
    return proj_cases(pro, epi, fmt)


def all_cases():
    return [c for r in ROLES for c in role_cases(*r)]


# ---------------------------------------------------------------------------------------------------- the persistent second trip
NOMINAL_CUS = 256


def persistent_shapes():
    """(pro, epi, fmt, variant) of every persistent instantiation"""
    return [(p, e, f, v) for (p, e, f), t in TABLE.items() for v, s in sorted(t.items()) if s[3]]


def persistent_case(pro, epi, fmt, variant, hd, cus):
    """K = 64 and a unit count that exceeds the grid's first round (CUs x blocks per CU x waves x R) by a ragged remainder: some waves
    take a second chunk, the others do not.  Returns (case, first_round_units)."""
    R, U, waves, bpc, KS = TABLE[(pro, epi, fmt)][variant]
    first = cus * bpc * waves * R
    tag = f"-persist{variant}"
    if epi == QKV:                       # H + 2 heads of hd / 2 units: one head and a half beyond the first round, or more
        per = hd // 2
        H = -(-first // per) - 1
        case = _case(pro, epi, fmt, 64, H=H, KVH=1, hd=hd, pos=POS_IN, tag=tag)
    elif epi == SWIGLU:
        ff = (first + 40 + 7) // 8 * 8
        ff += 8 * (ff % 7 == 0)          # (gate and up rows ff apart carry different fp8 scales)
        case = _case(pro, epi, fmt, 64, ff=ff, tag=tag)
    else:
        case = _case(pro, epi, fmt, 64, N=first + 37, tag=tag)
    return case, first
