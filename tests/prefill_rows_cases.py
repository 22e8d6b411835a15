"""Inputs and references of the prefill row-kernel and attention-layout op tests (tests/test_prefill_rows_host.py checks them on the CPU,
tests/test_gpu_prefill_rows.py feeds the same objects to dtk_op_rope_scatter / dtk_op_rows_norm / dtk_op_swiglu / dtk_op_attention_ex /
dtk_op_rows_move).

A case holds the host operands of ONE launch of a kernel of csrc/kernels_batched.hip that sits between the GEMMs of a prefill layer (or of
the ViT / the adapter's cross layer), the buffers it writes and two references:

  mode "f64": the operation on the exact operand values in float64 with the kernel's bf16 rounding points (the Linear's output, the SiLU,
              the normalised row, ...);
  mode "f32": the same chain on the oracle's own float32 lines — oracle.llama.rmsnorm / apply_rope / attention, oracle.vit.layernorm /
              im2col, oracle.ops.linear and the oracle's SwiGLU line rb(rb(silu(g)) * u).  The second legitimate reference: its distance
              from the first sets the bar of the chained outputs (MEASURED_CHAIN_*, asserted by the host test).

Every result buffer starts as a quiet NaN with a payload of its own, the gaps of strided INPUT buffers (rows >= Tk of a cache, the tail
of a row behind D, partial rows >= M) hold NaN too; judge() demands that every cell the kernel must not write keeps its bits.

Bars (none invented here).  "single": test_op_gemm's rel-L2 < 1e-3, <= 2.01 bf16 ulps, < 5 % differing — k_sk_reduce's C from partials
whose fp32 sums are exact.  "chain": min(test_op_attention's 4.01 ulps / 2e-3, 2 x the two-reference distance) — norms, SwiGLU, C behind a
residual.  "attn": test_op_attention's 2e-3 / 4.01.  "exact32": bit-equal to the float32 chain — q / k after RoPE (every step of
rope_scatter_row is one correctly rounded fp32 operation: products of two bf16 numbers are exact, the add rounds once, the slices are
added in slice order), which the float64 chain can miss only by the double rounding of that add.  "exact": bit-equal to the float64
reference — V (a bit copy: -0.0 and a NaN payload survive), gather, copy, im2col (one rounding of an fp32 pixel, ties included), and the
GRID cases: rows of +-1 under an RMSNorm with weights in eighths (mean square 1: x * rsqrt(1 + eps) rounds to +-1 whatever the last bits
of the rsqrt), for k_sk_reduce a residual of +-1 plus sums that the bf16 rounding of the add removes, and SwiGLU operands picked so that
SiLU(g) and the product sit at least 2^-6 ulp from a rounding boundary (an expf a few fp32 ulps off cannot move them) while rounding the
SiLU or not gives different results.

The mirrored thread-to-column maps at the end (rms_lane_trips, sk_thread_trips, silu_grid, g3_tile, ...) are what the coverage claims of
the host test are computed from."""
from __future__ import annotations

import numpy as np
import torch

from oracle.llama import apply_rope, attention, rmsnorm, rope_tables
from oracle.ops import bits_to_f32, f32_to_bits, linear, rb
from oracle.vit import im2col, layernorm
from tests.gemv_b_cases import ulp_report

EPS, LN_EPS = 1e-5, 1e-6
NAN_Q, NAN_K, NAN_V, NAN_Y, NAN_C, NAN_ACT, NAN_O, NAN_DST = 0x7FC1, 0x7FC2, 0x7FC3, 0x7FC4, 0x7FC5, 0x7FC6, 0x7FC7, 0x7FC8   # one payload per result buffer
NAN_IN, NAN_GAP = 0x7FD5, 0x7FE9         # a NaN among the V inputs (it must arrive with its payload); what input gaps hold
T_ROPE, T_MAX, MAX_POS = 5, 16, 32
DTK_EPI_BIAS, DTK_EPI_RESIDUAL, DTK_EPI_GATED_RESIDUAL = 1, 4, 8

SINGLE_RL2, SINGLE_ULPS, SINGLE_FRAC = 1e-3, 2.01, 0.05                 # test_op_gemm
ATTN_RL2, ATTN_ULPS = 2e-3, 4.01                                        # test_op_attention
# float64 vs float32 reference, worst over every case below, its redraws and short_row_distance(): 1.95 ulps (the GEMM_SWIGLU case M 257,
# ff 16, K 576: a flip of a gate's Linear output ahead of the SiLU), rel-L2 7.46e-3 (one flip of the normalised value in a row of 4; the
# case list itself stays at 1.6e-4).  Twice the rel-L2 is beyond the cap, so that bar IS the cap; the ulps bar is 3.9.
MEASURED_CHAIN_ULPS, MEASURED_CHAIN_RL2 = 1.95, 7.46e-3
CHAIN_ULPS, CHAIN_RL2 = min(ATTN_ULPS, 2 * MEASURED_CHAIN_ULPS), min(ATTN_RL2, 2 * MEASURED_CHAIN_RL2)

MUTATIONS = ("pos_off", "rope_sign", "rope_partner_interleaved", "row_and_position_swapped", "kv_head_shift", "v_rotated", "q_token_major",
             "slice_dropped", "slice_counted_twice", "eps_dropped", "mean_over_ld", "resid_dropped", "norm_before_resid_rounding",
             "gate_up_swap", "silu_unrounded", "last_pair_block_dropped", "gqa_modulo_map", "causal_off_by_one", "q_offset_ignored",
             "batch_stride_zero", "last_key_tile_dropped", "im2col_kh_kw_swapped", "gather_id_off")


def r64(x):
    """float64 -> the bf16 number nearest to it, as float64"""
    return x.to(torch.bfloat16).double()


def _bits(v):
    """values of a result (fp32 tensor of bf16 numbers, or bf16 bit patterns kept as uint16 so that a NaN payload survives) -> uint16"""
    if isinstance(v, np.ndarray):
        return v
    return f32_to_bits(v.float().contiguous())


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)))


def _worse(x, y):
    return float("nan") if (x != x or y != y) else max(x, y)


def slice_sum(part, S, mode, mutate=None):
    """part [S][rows][n] fp32 -> the slices' sum as the kernels form it: slice 0, + slice 1, ... in fp32 (float64: exactly)"""
    ks = list(range(S))
    if mutate == "slice_dropped":
        ks = ks[:-1]
    elif mutate == "slice_counted_twice":
        ks = ks + [S - 1]
    if mode == "f64":
        return sum(part[k].double() for k in ks)
    v = part[ks[0]].clone()
    for k in ks[1:]:
        v = v + part[k]
    return v


def rmsnorm64(x, w, eps, div=None):
    x = x.double()
    var = x.pow(2).sum(-1, keepdim=True) / (div or x.shape[-1])
    return rb((w.double() * r64(x * torch.rsqrt(var + eps))).float())


def swiglu(g, u, mode, unrounded=False):
    """the oracle's line act = rb(rb(silu(g)) * u) (float64: with the SiLU and the product in float64)"""
    if mode == "f64":
        s = g.double() / (1 + torch.exp(-g.double()))
        return rb(((s if unrounded else r64(s)) * u.double()).float())
    s = torch.nn.functional.silu(g)
    return rb((s if unrounded else rb(s)) * u)


class Case:
    group = ""
    ctor = None

    def kinds(self):
        raise NotImplementedError

    def ref(self, mode="f64"):
        """reference(mode), computed once"""
        memo = self.__dict__.setdefault("_memo", {})
        if mode not in memo:
            memo[mode] = self.reference(mode)
        return memo[mode]

    def write_mask(self):
        if "_mask" in self.__dict__:
            return self._mask
        ref = self.ref()
        fill = lambda c: {k: (np.full(_bits(v).shape, c, dtype=np.uint16) if k in self.kinds() else v) for k, v in ref.items()}
        a, b = self.place(fill(1)), self.place(fill(2))
        self._mask = {n: a[n] != b[n] for n in a}
        return self._mask

    def judge(self, got):
        """got = the buffers after the run.  Returns (ok, figures)."""
        want, init, mask = self.place(self.ref()), self.initial(), self.write_mask()
        fig = {"untouched": True, "exact": True, "single": (0.0, 0.0, 0.0), "chain": (0.0, 0.0), "attn": (0.0, 0.0)}
        w32 = None
        for name, kind in self.kinds().items():
            g, m = got[name].reshape(-1), mask[name].reshape(-1)
            if not np.array_equal(g[~m], init[name].reshape(-1)[~m]):
                fig["untouched"] = False
            w = want[name].reshape(-1)
            if kind == "exact32":
                w32 = w32 or self.place(self.ref("f32"))
                w = w32[name].reshape(-1)
            if kind in ("exact", "exact32"):
                if not np.array_equal(g[m], w[m]):
                    fig["exact"] = False
                continue
            rep = ulp_report(bits_to_f32(g[m]), bits_to_f32(w[m]))
            if kind == "single":
                fig["single"] = tuple(_worse(x, y) for x, y in zip(fig["single"], rep))
            else:
                fig[kind] = tuple(_worse(x, y) for x, y in zip(fig[kind], rep[1:]))
        fr, u, r = fig["single"]
        ok = fig["untouched"] and fig["exact"] and fr < SINGLE_FRAC and u <= SINGLE_ULPS and r < SINGLE_RL2 and \
            fig["chain"][0] <= CHAIN_ULPS and fig["chain"][1] < CHAIN_RL2 and fig["attn"][0] <= ATTN_ULPS and fig["attn"][1] < ATTN_RL2
        return bool(ok), fig

    def reference_distance(self):
        """worst (ulps, rel-L2) of the chained outputs between the float32 and the float64 reference"""
        a, b, mask = self.place(self.ref("f32")), self.place(self.ref()), self.write_mask()
        wu = wr = 0.0
        for name, kind in self.kinds().items():
            if kind == "chain":
                m = mask[name].reshape(-1)
                _, u, r = ulp_report(bits_to_f32(a[name].reshape(-1)[m]), bits_to_f32(b[name].reshape(-1)[m]))
                wu, wr = max(wu, u), max(wr, r)
        return wu, wr


# ---------------------------------------------------------------------------------------------------- RoPE, Q scatter, KV append
def rope64(x, cos, sin):
    h = x.shape[-1] // 2
    x, cos, sin = x.double(), cos.double(), sin.double()
    x1, x2 = x[..., :h], x[..., h:]
    return torch.cat([r64(r64(x1 * cos) + r64(-x2 * sin)), r64(r64(x2 * cos) + r64(x1 * sin))], dim=-1).float()


ROWS_TABLES = {"a": ([3, 4, 5, 3, 4], [8, 9, 10, 11, 12]),           # {position, cache row}: they differ, and the positions restart mid-table
               "b": ([6, 7, 8, 6, 7], [11, 12, 13, 14, 15])}        # ... ending at row T_MAX - 1
SLICE_MAG = (1.0, -4.0, 0.25, 2.0, -8.0, 0.5, -1.0, 16.0)           # slices of unequal magnitude and sign: order and count matter


class RopeCase(Case):
    """form 0: k_rope_scatter<hd> / k_rope_scatter_rows<hd> on bf16 QKV; S >= 1: k_sk_rope_scatter<S, hd> / _rows on fp32 partials"""
    group = "rope"

    def __init__(self, hd, H, KVH, start=3, table=None, S=0, seed=0):
        self.hd, self.H, self.KVH, self.start, self.table, self.S, self.T = hd, H, KVH, start, table, S, T_ROPE
        T, self.qkvn = T_ROPE, (H + 2 * KVH) * hd
        g = _gen(1, hd, H, KVH, start, S, len(table or ""), seed)
        self.cos, self.sin = rope_tables(hd, 10000.0, 1.0, MAX_POS)
        self.pos, self.row = (np.array(a) for a in (ROWS_TABLES[table] if table else ([start + t for t in range(T)],) * 2))
        v0 = (H + KVH) * hd
        if S == 0:
            self.qkv = f32_to_bits(rb(torch.randn(T, self.qkvn, generator=g)))
            self.qkv[1, v0 + 3], self.qkv[T - 1, self.qkvn - 1], self.qkv[2, v0 + hd // 2 + 1] = 0x8000, 0x8000, NAN_IN
        else:
            self.part_rows = T + 3            # (the product's stride is SK_CHUNK_ROWS rows: larger than the data)
            self.part = torch.full((S, self.part_rows, self.qkvn), float("nan"))
            for s in range(S):
                self.part[s, :T] = torch.randn(T, self.qkvn, generator=g) * SLICE_MAG[s] + 0.25 * SLICE_MAG[(s + 3) % 8]
            self.part[:, 1, v0 + 3] = -0.0

    @property
    def name(self):
        where = f"rows-{self.table}" if self.table else f"start{self.start}"
        return f"rope-hd{self.hd}-H{self.H}KVH{self.KVH}-{where}" + (f"-S{self.S}" if self.S else "-bf16")

    def kinds(self):
        return {"q": "exact32", "k": "exact32", "v": "exact" if self.S == 0 else "exact32"}      # (bf16 form: V is a bit copy; sliced: bf16 of the fp32 sum)

    def applies(self, m):
        return {"pos_off": True, "rope_sign": True, "rope_partner_interleaved": True, "row_and_position_swapped": self.table is not None,
                "kv_head_shift": True, "v_rotated": True, "q_token_major": self.H > 1, "slice_dropped": self.S >= 2,
                "slice_counted_twice": self.S >= 1}.get(m, False)

    def x_bits(self, mode="f64", mutate=None):
        """the kernel's input row as bf16 bits [T][qkvn]: QKV itself, or bf16(sum of slices)"""
        if self.S == 0:
            return self.qkv
        v = slice_sum(self.part[:, :self.T], self.S, mode, mutate)
        return f32_to_bits(v.to(torch.bfloat16).float())

    def reference(self, mode="f64", mutate=None):
        T, H, KVH, hd = self.T, self.H, self.KVH, self.hd
        bits = self.x_bits(mode, mutate).reshape(T, H + 2 * KVH, hd).transpose(1, 0, 2)      # [heads][T][hd]
        x = bits_to_f32(np.ascontiguousarray(bits)).reshape(H + 2 * KVH, T, hd)
        pos, row = self.pos, self.row
        if mutate == "pos_off":
            pos = pos + 1
        elif mutate == "row_and_position_swapped":
            pos, row = row, pos
        cos, sin = self.cos[pos], self.sin[pos]
        if mutate == "rope_sign":
            sin = -sin
        rope = rope64 if mode == "f64" else apply_rope
        if mutate == "rope_partner_interleaved":       # the pair (2i, 2i + 1) instead of (i, i + hd/2)
            perm = torch.cat([torch.arange(0, hd, 2), torch.arange(1, hd, 2)])
            inv = torch.argsort(perm)
            plain = rope
            rope = lambda t, c, s: plain(t[..., perm], c, s)[..., inv]
        k0 = H - 1 if mutate == "kv_head_shift" else H          # the k section taken one head early
        q, k = rope(x[:H], cos, sin), rope(x[k0:k0 + KVH], cos, sin)
        v = np.ascontiguousarray(bits[H + KVH:])
        if mutate == "v_rotated":
            v = f32_to_bits(rope(torch.nan_to_num(x[H + KVH:]), cos, sin))
        if mutate == "q_token_major":
            q = q.permute(1, 0, 2).reshape(H, T, hd)
        return {"q": q, "k": k, "v": v, "row": row}

    def initial(self):
        kv = (self.KVH, T_MAX, self.hd)
        return {"q": np.full((self.H, self.T, self.hd), NAN_Q, dtype=np.uint16), "k": np.full(kv, NAN_K, dtype=np.uint16), "v": np.full(kv, NAN_V, dtype=np.uint16)}

    def place(self, out):
        buf = self.initial()
        buf["q"][:] = _bits(out["q"])
        buf["k"][:, out["row"]] = _bits(out["k"])
        buf["v"][:, out["row"]] = _bits(out["v"])
        return buf


# ---------------------------------------------------------------------------------------------------- norms behind a role
class NormCase(Case):
    """form 0 k_rmsnorm_rows, 1 k_rmsnorm_rows_sk, 3 k_layernorm_rows: X [M][ldx] -> Y [M][ldy]"""
    group = "norm"

    def __init__(self, form, M, D, ldx=None, ldy=None, style="random", in_place=False, seed=0):
        self.form, self.M, self.D, self.style, self.in_place = form, M, D, style, in_place
        pad = 8 if form != 1 else 2
        self.ldx, self.ldy = (D if in_place else (ldx or D + pad)), (D if in_place else (ldy or D))
        g = _gen(2, form, M, D, self.ldx, self.ldy, len(style), seed)
        if style == "grid":
            self.x = (torch.randint(0, 2, (M, D), generator=g) * 2 - 1).float()
            self.w = torch.randint(-16, 17, (D,), generator=g).float() / 8
        elif form == 3:
            self.x = rb(torch.randn(M, D, generator=g) * 3 + 0.5)
            self.w = rb(1 + 0.1 * torch.randn(D, generator=g))
        else:
            self.x = rb(torch.randn(M, D, generator=g))
            self.w = rb(1 + 0.1 * torch.randn(D, generator=g))
            self.x[M // 2] = self.x[M // 2] * 2.0 ** -10          # a row so small that eps decides its result
        self.b = rb(0.1 * torch.randn(D, generator=g)) if form == 3 else None
        self.has_tiny = style == "random" and form != 3

    @property
    def name(self):
        return f"norm-form{self.form}-M{self.M}-D{self.D}-ldx{self.ldx}-ldy{self.ldy}-{self.style}" + ("-inplace" if self.in_place else "")

    def kinds(self):
        return {"y": "exact" if self.style == "grid" else "chain"}

    def applies(self, m):
        # (a mean over ldx scales the row by sqrt(ldx / D): below 1 % of padding that is inside any bf16 bar, and no GRID row moves)
        return {"eps_dropped": self.has_tiny, "mean_over_ld": self.ldx > 1.01 * self.D}.get(m, False)

    def x_buffer(self):
        buf = np.full((self.M, self.ldx), NAN_GAP, dtype=np.uint16)
        buf[:, :self.D] = f32_to_bits(self.x)
        return buf

    def reference(self, mode="f64", mutate=None):
        div = self.ldx if mutate == "mean_over_ld" else self.D
        if self.form == 3:
            if mode == "f32" and mutate is None:
                return {"y": layernorm(self.x, self.w, self.b, LN_EPS)}
            x = self.x.double()
            mean = x.sum(-1, keepdim=True) / div
            var = (x - mean).pow(2).sum(-1, keepdim=True) / div
            return {"y": rb(((x - mean) * torch.rsqrt(var + LN_EPS) * self.w.double() + self.b.double()).float())}
        eps = 0.0 if mutate == "eps_dropped" else EPS
        if mode == "f32" and mutate is None:
            return {"y": rmsnorm(self.x, self.w, eps)}
        return {"y": rmsnorm64(self.x, self.w, eps, div)}

    def initial(self):
        return {"y": self.x_buffer() if self.in_place else np.full((self.M, self.ldy), NAN_Y, dtype=np.uint16)}

    def place(self, out):
        buf = self.initial()
        buf["y"][:, :self.D] = _bits(out["y"])
        return buf


SK_FLAGS = (0, DTK_EPI_RESIDUAL, DTK_EPI_BIAS | DTK_EPI_RESIDUAL)


class SkCase(Case):
    """form 2: k_sk_reduce<S> on fp32 partials [S][part_rows][N] -> C [M][ldc] (+ the fused RMSNorm -> Y [M][ldy])"""
    group = "sk_reduce"

    def __init__(self, S, N, norm, flags, mis, style="random", M=3, seed=0):
        self.S, self.N, self.norm, self.flags, self.mis, self.M = S, N, norm, flags, mis, M
        self.style = style = "exact" if (flags == 0 and style == "random") else style
        pad = 2 if mis else 4                  # ld = N + 2: neither 8-byte stores nor 8-byte loads of a row (the scalar paths)
        self.ldc, self.ldr, self.ldy, self.part_rows = N + pad, N + pad, N + pad, M + 2
        g = _gen(3, S, N, norm, flags, mis, len(style), seed)
        self.part = torch.full((S, self.part_rows, N), float("nan"))
        self.bias = rb(0.1 * torch.randn(N, generator=g))
        self.res = rb(torch.randn(M, N, generator=g))
        self.w = rb(1 + 0.1 * torch.randn(N, generator=g))
        self.gate = rb(torch.tensor([0.75]))            # DTK_EPI_GATED_RESIDUAL: the logit of the adapter's gate
        if style == "exact":        # multiples of 2^-6 below 2^8: every fp32 sum of up to 8 of them is exact, so C has one rounding
            for s in range(S):
                self.part[s, :M] = torch.randint(-2 ** 11, 2 ** 11, (M, N), generator=g).float() / 64 * 2.0 ** (s % 3)
        elif style == "grid":
            # residual +-1; the slices sum (exactly) to +-(2^-8 - 2^-14) towards the residual's side on 3 columns of 4, to 0 on the
            # fourth: bf16(res + sum) = +-1, mean square 1, Y = +-w.  A norm of the unrounded sum moves the fourth columns by an ulp.
            assert flags == DTK_EPI_RESIDUAL and norm
            self.res = (torch.randint(0, 2, (M, N), generator=g) * 2 - 1).float()
            self.w = torch.randint(-16, 17, (N,), generator=g).float() / 8
            unit = 2.0 ** -14
            tot = torch.where(torch.arange(N) % 4 == 3, 0.0, 63.0)[None, :] * self.res
            rest = torch.randint(-3, 4, (S, M, N), generator=g).float()
            rest[0] = tot - rest[1:].sum(0)
            self.part[:, :M] = rest * unit
        else:
            for s in range(S):
                self.part[s, :M] = torch.randn(M, N, generator=g) * abs(SLICE_MAG[s]) * 0.25

    @property
    def name(self):
        return f"sk-S{self.S}-N{self.N}-{'norm' if self.norm else 'plain'}-flags{self.flags}-{'mis' if self.mis else 'al'}-{self.style}"

    def kinds(self):
        k = {"c": "exact" if self.style == "grid" else ("single" if self.flags == 0 else "chain")}
        if self.norm:
            k["y"] = "exact" if self.style == "grid" else "chain"
        return k

    def applies(self, m):
        return {"slice_dropped": self.S >= 2, "slice_counted_twice": True, "resid_dropped": bool(self.flags & DTK_EPI_RESIDUAL),
                "norm_before_resid_rounding": self.style == "grid"}.get(m, False)

    def res_buffer(self):
        buf = np.full((self.M, self.ldr), NAN_GAP, dtype=np.uint16)
        buf[:, :self.N] = f32_to_bits(self.res)
        return buf

    def reference(self, mode="f64", mutate=None):
        f64 = mode == "f64"
        v = slice_sum(self.part[:, :self.M], self.S, mode, mutate)
        if self.flags & DTK_EPI_BIAS:
            v = v + (self.bias.double() if f64 else self.bias)
        c = r64(v) if f64 else rb(v)
        if self.flags & DTK_EPI_GATED_RESIDUAL:         # bf16(bf16(sigmoid(gate)) * the Linear's output)
            gs = r64(1 / (1 + torch.exp(-self.gate.double()))) if f64 else rb(torch.sigmoid(self.gate))
            c = r64(gs * c) if f64 else rb(gs * c)
        pre = c
        if (self.flags & DTK_EPI_RESIDUAL) and mutate != "resid_dropped":
            pre = (self.res.double() if f64 else self.res) + c
            c = r64(pre) if f64 else rb(pre)
        out = {"c": c.float()}
        if self.norm:
            x = pre if mutate == "norm_before_resid_rounding" else c
            out["y"] = rmsnorm64(x, self.w, EPS) if f64 else rmsnorm(x, self.w, EPS)
        return out

    def initial(self):
        buf = {"c": np.full((self.M, self.ldc), NAN_C, dtype=np.uint16)}
        if self.norm:
            buf["y"] = np.full((self.M, self.ldy), NAN_Y, dtype=np.uint16)
        return buf

    def place(self, out):
        buf = self.initial()
        for n in buf:
            buf[n][:, :self.N] = _bits(out[n])
        return buf


# ---------------------------------------------------------------------------------------------------- SwiGLU in three forms
def _margin(x):
    """distance (in ulps of its bf16 neighbourhood) of a float64 value from the nearest bf16 rounding boundary"""
    ulp = torch.exp2(torch.floor(torch.log2(x.abs())) - 7)
    return 0.5 - (x - r64(x)).abs() / ulp


def swiglu_exact_pairs(n, g):
    """n (gate, up) pairs of bf16 numbers whose SiLU and whose product both sit >= 2^-6 ulp from a rounding boundary, and for which
    rounding the SiLU to bf16 first (as the kernels and the oracle do) gives another result than not rounding it"""
    gate = rb(torch.rand(200 * n + 4000, generator=g) * 16 - 8)
    up = rb(torch.randn(gate.numel(), generator=g))
    s = gate.double() / (1 + torch.exp(-gate.double()))
    pr, pu = r64(s) * up.double(), s * up.double()
    ok = (gate.abs() > 0.05) & (up.abs() > 0.05) & (_margin(s) > 2.0 ** -6) & (_margin(pr) > 2.0 ** -6) & (_margin(pu) > 2.0 ** -6) & (r64(pr) != r64(pu))
    idx = torch.nonzero(ok).reshape(-1)[:n]
    assert idx.numel() == n, (n, int(ok.sum()))
    return gate[idx], up[idx]


class SwiCase(Case):
    """form 0 k_silu_mul on GU [M][2 ff]; 1 k_sk_reduce_swiglu<S> on partials [S][part_rows][2 ff]; 2 k_gemm_g3's GEMM_SWIGLU epilogue on
    A [M][K], W [2 ff][K]"""
    group = "swiglu"

    def __init__(self, form, M, ff, S=0, K=0, style="random", seed=0):
        self.form, self.M, self.ff, self.S, self.K, self.style = form, M, ff, S, K, style
        self.ldact = ff if form == 0 else ff + 4
        g = _gen(4, form, M, ff, S, K, len(style), seed)
        if form == 2:
            self.A = rb(torch.randn(M, K, generator=g))
            self.W = rb(torch.randn(2 * ff, K, generator=g) * 3 * K ** -0.5)
            return
        if style == "grid":
            gate, up = (t.reshape(M, ff) for t in swiglu_exact_pairs(M * ff, g))
        else:       # gates over -20 .. 20: both SiLU tails
            gate, up = rb(torch.rand(M, ff, generator=g) * 40 - 20), rb(torch.randn(M, ff, generator=g))
        gu = torch.cat([gate, up], dim=1)
        if form == 0:
            self.GU = gu
            return
        self.part_rows = M + 2
        self.part = torch.full((S, self.part_rows, 2 * ff), float("nan"))
        if style == "grid":         # slice 0 = the value, then (S even: a 0 and) +0.5 / -0.5 in turn: every fp32 sum is exact
            self.part[0, :M] = gu
            for s, e in enumerate(([0.0] if (S - 1) % 2 else []) + [0.5, -0.5] * ((S - 1) // 2)):
                self.part[s + 1, :M] = e
        else:
            rest = torch.randn(S, M, 2 * ff, generator=g) * torch.tensor([abs(m) for m in SLICE_MAG[:S]])[:, None, None]
            rest[0] = gu - rest[1:].sum(0)
            self.part[:, :M] = rest

    @property
    def name(self):
        extra = {0: "", 1: f"-S{self.S}", 2: f"-K{self.K}"}[self.form]
        return f"swiglu-form{self.form}-M{self.M}-ff{self.ff}{extra}-{self.style}"

    def kinds(self):
        return {"act": "exact" if self.style == "grid" else "chain"}

    def applies(self, m):
        return {"gate_up_swap": True, "silu_unrounded": self.style == "grid", "last_pair_block_dropped": self.form == 2,
                "slice_dropped": self.form == 1 and self.S >= 2, "slice_counted_twice": self.form == 1}.get(m, False)

    def gate_up(self, mode="f64", mutate=None):
        """the bf16 [M][2 ff] the activation is taken of"""
        if self.form == 0:
            return self.GU
        if self.form == 1:
            return slice_sum(self.part[:, :self.M], self.S, mode, mutate).to(torch.bfloat16).float()
        if mode == "f64":
            return rb((self.A.double() @ self.W.double().t()).float())
        return linear(self.A, self.W)

    def reference(self, mode="f64", mutate=None):
        gu = self.gate_up(mode, mutate)
        gate, up = gu[:, :self.ff], gu[:, self.ff:]
        if mutate == "gate_up_swap":
            gate, up = up, gate
        act = swiglu(gate, up, mode, unrounded=mutate == "silu_unrounded")
        if mutate == "last_pair_block_dropped":
            per = g3_tile(self.M, 2 * self.ff)[1] // 2         # channels of a pair-ordered column block
            act = act.clone()
            act[:, (self.ff - 1) // per * per:] = float("nan")
        return {"act": act}

    def initial(self):
        return {"act": np.full((self.M, self.ldact), NAN_ACT, dtype=np.uint16)}

    def place(self, out):
        buf = self.initial()
        buf["act"][:, :self.ff] = _bits(out["act"])
        return buf


# ---------------------------------------------------------------------------------------------------- attention in the product's layouts
def attention64(q, k, v, scale, causal_offset=None):
    q, k, v = q.double(), k.double(), v.double()
    s = (q @ k.transpose(-1, -2)) * scale
    if causal_offset is not None:
        qpos = torch.arange(q.shape[1])[:, None] + causal_offset
        s = s.masked_fill(torch.arange(k.shape[1])[None, :] > qpos, float("-inf"))
    return rb((torch.softmax(s, dim=-1) @ v).float())


class AttnCase(Case):
    """launch_attention with the strides of a product call site.  Logical operands: q [Bq][H][Tq][hd], k / v [Bk][KVH][Tk][hd]; query
    head h reads K / V head h // G; causal: query i sits at position q_offset + i."""
    group = "attn"

    def __init__(self, layout, hd, H, G, Tq, Tk, nbatch, causal=0, q_offset=0, seed=0):
        self.layout, self.hd, self.H, self.G, self.Tq, self.Tk, self.B, self.causal, self.q_offset = layout, hd, H, G, Tq, Tk, nbatch, causal, q_offset
        self.KVH = H // G
        g = _gen(5, len(layout), hd, H, G, Tq, Tk, nbatch, causal, q_offset, seed)
        Bq, Bk = (1 if layout == "pool" else nbatch), (1 if layout == "cross" else nbatch)
        self.q = rb(torch.randn(Bq, H, Tq, hd, generator=g))
        self.k = rb(torch.randn(Bk, self.KVH, Tk, hd, generator=g))
        self.v = rb(torch.randn(Bk, self.KVH, Tk, hd, generator=g))
        D, B = H * hd, nbatch
        # per operand: (base, head stride, token stride, batch stride); elements of the raw buffer it lives in
        if layout == "prefill":         # Q head-major, caches with a T_max head stride, O token-major with ldo > H hd
            tm, ldo = Tk + 3, D + 8
            self.lay = {"q": (0, Tq * hd, hd, H * Tq * hd), "k": (0, tm * hd, hd, self.KVH * tm * hd), "v": (0, tm * hd, hd, self.KVH * tm * hd),
                        "o": (0, hd, ldo, Tq * ldo)}
            self.size = {"q": B * H * Tq * hd, "k": B * self.KVH * tm * hd, "v": B * self.KVH * tm * hd, "o": B * Tq * ldo}
        elif layout == "vit":           # interleaved [N][3 D] rows
            assert Tq == Tk and G == 1
            self.lay = {n: (i * D, hd, 3 * D, Tq * 3 * D) for i, n in enumerate("qkv")}
            self.lay["o"] = (0, hd, D, Tq * D)
            self.size = {"q": B * Tq * 3 * D, "k": B * Tq * 3 * D - D, "v": B * Tq * 3 * D - 2 * D, "o": B * Tq * D}
        elif layout == "cross":         # K / V of the few text tokens shared by the batch
            self.lay = {"q": (0, hd, D, Tq * D), "k": (0, hd, D, 0), "v": (0, hd, D, 0), "o": (0, hd, D, Tq * D)}
            self.size = {"q": B * Tq * D, "k": Tk * D, "v": Tk * D, "o": B * Tq * D}
        elif layout == "pool":          # one probe query for the whole batch, K / V interleaved [Tk][2 D]
            assert Tq == 1
            self.lay = {"q": (0, hd, D, 0), "k": (0, hd, 2 * D, Tk * 2 * D), "v": (D, hd, 2 * D, Tk * 2 * D), "o": (0, hd, D, D)}
            self.size = {"q": D, "k": B * Tk * 2 * D, "v": B * Tk * 2 * D - D, "o": B * D}
        else:
            raise ValueError(layout)

    @property
    def name(self):
        return f"attn-{self.layout}-hd{self.hd}-H{self.H}G{self.G}-{self.Tq}x{self.Tk}-B{self.B}" + (f"-causal{self.q_offset}" if self.causal else "")

    def kinds(self):
        return {"o": "attn"}

    def applies(self, m):
        last_tile = (self.Tk - 1) // 64 * 64
        return {"gqa_modulo_map": self.G > 1 and self.KVH > 1, "causal_off_by_one": bool(self.causal) and self.q_offset + 1 < self.Tk, "q_offset_ignored": bool(self.causal) and self.q_offset > 0,
                "batch_stride_zero": self.B > 1 and self.layout != "cross",
                "last_key_tile_dropped": last_tile > 0 and (not self.causal or self.q_offset + self.Tq > last_tile)}.get(m, False)

    def strides(self):
        """{q_sh, q_st, q_sb, k_sh, ...} as dtk_op_attention_ex takes them"""
        return np.array([self.lay[n][i] for n in "qkvo" for i in (1, 2, 3)], dtype=np.int64)

    def _index(self, n, nb, nh, nt):
        base, sh, st, sb = self.lay[n]
        b, h, t, e = np.ogrid[:nb, :nh, :nt, :self.hd]
        return b * sb + h * sh + t * st + e          # (the base is applied by taking the operand's pointer that far in)

    def operands(self):
        """raw buffers as the entry point takes them (the pointer of an interleaved operand already moved to its base), gaps = NaN"""
        out = {}
        if self.layout in ("vit", "pool"):        # q / k / v (k / v) share ONE interleaved buffer: build it once, then take the views
            names = "qkv" if self.layout == "vit" else "kv"
            whole = np.full(self.size[names[0]], NAN_GAP, dtype=np.uint16)
            for n in names:
                t = getattr(self, n)
                whole[self.lay[n][0] + self._index(n, *t.shape[:3])] = f32_to_bits(t)
            for n in names:
                out[n] = whole[self.lay[n][0]:]
                assert out[n].size == self.size[n]
            if self.layout == "vit":
                assert not (whole == NAN_GAP).any()
        for n in "qkv":
            if n not in out:
                t = getattr(self, n)
                out[n] = np.full(self.size[n], NAN_GAP, dtype=np.uint16)
                out[n][self._index(n, *t.shape[:3])] = f32_to_bits(t)
        return out

    def reference(self, mode="f64", mutate=None):
        att = attention64 if mode == "f64" else attention
        off = self.q_offset if self.causal else None
        if mutate == "causal_off_by_one":
            off += 1
        elif mutate == "q_offset_ignored":
            off = 0
        heads = [(h % self.KVH if mutate == "gqa_modulo_map" else h // self.G) for h in range(self.H)]
        tk = (self.Tk - 1) // 64 * 64 if mutate == "last_key_tile_dropped" else self.Tk
        outs = []
        for b in range(self.B):
            bk = 0 if mutate == "batch_stride_zero" else b % self.k.shape[0]
            outs.append(att(self.q[b % self.q.shape[0]], self.k[bk][heads][:, :tk], self.v[bk][heads][:, :tk], self.hd ** -0.5, off))
        return {"o": torch.stack(outs)}

    def initial(self):
        return {"o": np.full(self.size["o"], NAN_O, dtype=np.uint16)}

    def place(self, out):
        buf = self.initial()
        buf["o"][self._index("o", self.B, self.H, self.Tq)] = _bits(out["o"]).reshape(self.B, self.H, self.Tq, self.hd)
        return buf


# ---------------------------------------------------------------------------------------------------- gather, copy, im2col
class MoveCase(Case):
    """form 0 k_embed_gather, 1 k_copy_rows, 2 k_im2col"""
    group = "move"

    def __init__(self, form, D=0, ldp=0, seed=0):
        self.form, self.D, self.ldp = form, D, ldp
        g = _gen(6, form, D, ldp, seed)
        if form == 0:
            self.V = 7
            self.ids = np.array([0, 6, 3, 3, 0, 6, 5], dtype=np.int32)        # 0, V - 1 and repeats
            self.M = len(self.ids)
            self.table = f32_to_bits(rb(torch.randn(self.V, D, generator=g)))
        elif form == 1:
            self.M, self.lds, self.ldd = 3, D + 8, D + 16
            self.src = np.full((self.M, self.lds), NAN_GAP, dtype=np.uint16)
            self.src[:, :D] = f32_to_bits(rb(torch.randn(self.M, D, generator=g)))
            self.src[1, 0], self.src[2, D - 1] = 0x8000, NAN_IN
        else:
            self.image, self.patch = 28, 14
            base = rb(torch.randn(3, 28, 28, generator=g))
            ulp = torch.exp2(torch.floor(torch.log2(base.abs().clamp(min=2.0 ** -20))) - 7)
            frac = torch.tensor([0.5, 0.25, -0.5, 0.75, 0.0, -0.25, 0.4999])[torch.randint(0, 7, base.shape, generator=g)]
            self.pixels = (base + frac * ulp).float()        # not bf16 numbers; |frac| = 0.5: ties
            assert bool((rb(self.pixels) != self.pixels).float().mean() > 0.7)

    @property
    def name(self):
        return {0: f"gather-d{self.D}", 1: f"copy-D{self.D}", 2: f"im2col-ldp{self.ldp}"}[self.form]

    def kinds(self):
        return {"dst": "exact"}

    def applies(self, m):
        return {"gather_id_off": self.form == 0, "im2col_kh_kw_swapped": self.form == 2}.get(m, False)

    def reference(self, mode="f64", mutate=None):
        if self.form == 0:
            ids = (self.ids + 1) % self.V if mutate == "gather_id_off" else self.ids
            return {"dst": self.table[ids]}
        if self.form == 1:
            return {"dst": self.src[:, :self.D].copy()}
        px = self.pixels.transpose(1, 2) if mutate == "im2col_kh_kw_swapped" else self.pixels
        cols = im2col(px, self.patch)
        if mutate == "im2col_kh_kw_swapped":            # the transposed image's patches come out in (px, py) order: put them back
            n = self.image // self.patch
            cols = cols.reshape(n, n, -1).transpose(0, 1).reshape(n * n, -1)
        pad = torch.zeros(cols.shape[0], self.ldp - cols.shape[1])
        return {"dst": torch.cat([rb(cols), pad], dim=1)}

    def initial(self):
        shape = {0: (getattr(self, "M", 0), self.D), 1: (3, self.D + 16), 2: (4, self.ldp)}[self.form]
        return {"dst": np.full(shape, NAN_DST, dtype=np.uint16)}

    def place(self, out):
        buf = self.initial()
        v = _bits(out["dst"])
        buf["dst"][:, :v.shape[1]] = v
        return buf


# ---------------------------------------------------------------------------------------------------- the case lists
_cache = {}


def _case(cls, *a, **kw):
    key = (cls, a, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = cls(*a, **kw)
        _cache[key].ctor = (cls, a, kw)
    return _cache[key]


HEADS = ((4, 4), (4, 2), (4, 1), (1, 1))
STARTS = (3, 11)                       # 11 ends at row T_MAX - 1; never position 0 alone (sin = 0 would hide a RoPE sign)


def rope_cases():
    out = []
    for hd in (128, 64):
        for i, (H, KVH) in enumerate(HEADS):
            out += [_case(RopeCase, hd, H, KVH, start=s) for s in STARTS]
            out.append(_case(RopeCase, hd, H, KVH, table="ab"[i % 2]))
        for S in range(1, 9):          # every <S, hd> of both sliced kernels
            H, KVH = HEADS[S % 4]
            out.append(_case(RopeCase, hd, H, KVH, start=STARTS[S % 2], S=S))
            H, KVH = HEADS[(S + 1) % 4]
            out.append(_case(RopeCase, hd, H, KVH, table="ab"[S % 2], S=S))
    return out


RMS_D = (8, 72, 520, 2048, 4096)
SK_ROWS_N = (4, 2048, 4096, 4100)
SK_N = (4, 260, 4096, 4100, 8200)


def norm_cases():
    out = []
    for form, sizes in ((0, RMS_D), (1, SK_ROWS_N)):
        pad = 8 if form == 0 else 2
        for i, D in enumerate(sizes):
            out += [_case(NormCase, form, 1, D), _case(NormCase, form, 5, D, ldy=D + pad * (i % 2))]
        out += [_case(NormCase, form, 5, D, style="grid") for D in sizes[1::2] + sizes[-1:]]
    out.append(_case(NormCase, 3, 6, 72, in_place=True))
    out.append(_case(NormCase, 3, 5, 1152))
    return list(dict.fromkeys(out))


def sk_cases():
    out = []
    for norm in (1, 0):
        for S in range(1, 9):
            for j in range(2):
                i = 2 * (S - 1) + j + norm
                out.append(_case(SkCase, S, SK_N[i % 5], norm, SK_FLAGS[i % 3], (i // 3) % 2))
    for N in (4096, 4100, 8200):       # both alignments on both sides of the keep[] / read-back branch, every flag set
        for mis in (0, 1):
            out += [_case(SkCase, 3 + mis, N, 1, f, mis) for f in SK_FLAGS]
    out += [_case(SkCase, 2 + 5 * mis, 260, 1 - mis, DTK_EPI_BIAS | DTK_EPI_RESIDUAL | DTK_EPI_GATED_RESIDUAL, mis) for mis in (0, 1)]
    out += [_case(SkCase, S, N, 1, DTK_EPI_RESIDUAL, mis, style="grid") for S, N, mis in ((1, 260, 0), (5, 260, 1), (4, 4100, 0), (8, 4100, 1))]
    return list(dict.fromkeys(out))


SILU_FF, SKSWI_FF = (8, 24, 88, 5504), (4, 24, 4096, 4100)
G3_K, G3_FF, G3_M = (128, 136, 200, 576), (16, 64, 80, 144), (1, 100, 129, 257)
SILU_BIG = (1030, 8200)                # 1,055,750 chunks > 4096 blocks x 256 threads: the smallest shape whose grid-stride loop turns


def swiglu_cases(form=None):
    f0 = [_case(SwiCase, 0, M, ff) for ff in SILU_FF for M in (1, 5)] + [_case(SwiCase, 0, *SILU_BIG)]
    f0 += [_case(SwiCase, 0, 5, 88, style="grid"), _case(SwiCase, 0, 1, 24, style="grid")]
    f1 = [_case(SwiCase, 1, 3, SKSWI_FF[(S + j) % 4], S=S) for S in range(1, 9) for j in (0, 2)]
    f1 += [_case(SwiCase, 1, 3, 24, S=S, style="grid") for S in (3, 6)]
    f2 = [_case(SwiCase, 2, G3_M[(i + j) % 4], ff, K=K) for i, K in enumerate(G3_K) for j, ff in enumerate(G3_FF)]
    return {None: f0 + f1 + f2, 0: f0, 1: f1, 2: f2}[form]


def attn_cases():
    P = lambda *a, **kw: _case(AttnCase, "prefill", *a, causal=1, **kw)
    out = [P(128, 4, 1, 1, 1, 1, q_offset=0), P(128, 4, 2, 17, 64, 1, q_offset=47), P(128, 4, 4, 65, 65, 1, q_offset=0),
           P(128, 4, 2, 65, 130, 3, q_offset=65), P(128, 4, 4, 1, 130, 1, q_offset=129), P(128, 2, 2, 1, 5, 3, q_offset=4),
           P(64, 4, 1, 17, 65, 1, q_offset=48), P(64, 4, 2, 65, 65, 3, q_offset=0), P(64, 4, 4, 17, 130, 1, q_offset=113),
           P(64, 2, 2, 1, 64, 1, q_offset=63), P(64, 4, 4, 65, 130, 1, q_offset=65), P(64, 4, 1, 5, 5, 3, q_offset=0)]
    out += [_case(AttnCase, "vit", 72, 2, 1, 65, 65, 3), _case(AttnCase, "vit", 72, 2, 1, 17, 17, 1), _case(AttnCase, "vit", 72, 1, 1, 130, 130, 1)]
    out += [_case(AttnCase, "cross", 72, 2, 1, Tq, 5, B) for Tq, B in ((17, 3), (65, 1), (1, 3))]
    out += [_case(AttnCase, "pool", 72, 2, 1, 1, Tk, B) for Tk, B in ((64, 3), (65, 1), (130, 3), (1, 3), (5, 1))]
    return out


def move_cases():
    return [_case(MoveCase, 0, D=d) for d in (8, 2056)] + [_case(MoveCase, 1, D=d) for d in (8, 2056)] + [_case(MoveCase, 2, ldp=l) for l in (592, 600)]


GROUPS = {"rope": rope_cases, "norm": norm_cases, "sk_reduce": sk_cases, "swiglu": swiglu_cases, "attn": attn_cases, "move": move_cases}


def all_cases():
    return [c for f in GROUPS.values() for c in f()]


DISTANCE_DRAWS = 6


def redraws(case):
    """the case on other operand draws: not run anywhere, they only widen the sample the distance between the two references is taken
    over (two legitimate orders differ by a rounding flip about once in 10^4 outputs)"""
    if "chain" not in case.kinds().values() or case.ctor is None:
        return []
    cls, a, kw = case.ctor
    if isinstance(case, SwiCase) and case.M * case.ff > 1e5:
        return []
    return [cls(*a, **{**kw, "seed": s}) for s in range(1, DISTANCE_DRAWS)]


SHORT_ROWS = 200000


def short_row_distance():
    """redraws of the shortest norm cases (M = 1, D = 4 and 8) by the hundred thousand, as the rows of one tall draw: a row is a case of
    its own (nothing crosses rows).  The two references differ by a rounding flip about once in 3 x 10^4 outputs (an fp32 product
    against a float64 one at a bf16 boundary 2^-8 wide), which the case list and a handful of redraws never meet in a row of 4 — where
    one flip is up to 2^-8 of a quarter of the outputs, the largest rel-L2 a legitimate result can be away.  Returns the worst
    (ulps, rel-L2) over the rows, each row judged alone (ulps floored at 1 % of the ROW's largest magnitude, as ulp_report does)."""
    wu = wr = 0.0
    for D in (4, 8):
        g = _gen(7, D)
        x, w = rb(torch.randn(SHORT_ROWS, D, generator=g)), rb(1 + 0.1 * torch.randn(D, generator=g))
        a, b = rmsnorm(x, w, EPS), rmsnorm64(x, w, EPS)
        diff = (a - b).abs()
        ulp = torch.maximum(b.abs(), 1e-2 * b.abs().amax(-1, keepdim=True) + 1e-30) * 2.0 ** -7
        wu = max(wu, float((diff / ulp).max()))
        wr = max(wr, float(((a - b).double().pow(2).sum(-1) / b.double().pow(2).sum(-1)).sqrt().max()))
    return wu, wr


# ---------------------------------------------------------------------------------------------------- the mirrored maps
def rms_lane_trips(D):
    """k_rmsnorm_rows / k_layernorm_rows: trips of each of a row's 64 lanes over its 16-byte chunks (for c = lane; c < D / 8; c += 64)"""
    return [len(range(lane, D // 8, 64)) for lane in range(64)]


def rows_per_block_tail(M):
    """rows of the last 4-row block of k_rmsnorm_rows / k_layernorm_rows"""
    return (M - 1) % 4 + 1


def sk_thread_trips(N, norm=True, by=0):
    """k_sk_reduce / k_rmsnorm_rows_sk: trips of thread 0 and of the last thread that has any (for n = nbeg + tid * 4; n < nend; n += 4096)"""
    nbeg = 0 if norm else by * 4096
    nend = N if norm else min(N, nbeg + 4096)
    trips = [len(range(nbeg + t * 4, nend, 4096)) for t in range(1024)]
    return max(trips), min(t for t in trips if t) if any(trips) else 0


def sk_reduce_grid_y(N, norm):
    return 1 if norm else (N + 4095) // 4096


def sk_norm_branch(N):
    """the fused norm of k_sk_reduce: the row stays in keep[] or is read back from the thread's own stores"""
    return "keep" if N <= 4096 else "readback"


def sk_vector_paths(case):
    """(C, residual, Y) take 8-byte accesses (operands are 256-byte aligned in the op scratch)"""
    return case.ldc % 4 == 0, case.ldr % 4 == 0, case.ldy % 4 == 0


def silu_grid(M, ff):
    """k_silu_mul: (blocks, chunks, whether a thread takes a second trip)"""
    total = M * (ff // 8)
    grid = max(1, min(4096, (total + 255) // 256))
    return grid, total, total > grid * 256


def sk_swiglu_grid_y(ff):
    return (ff + 4095) // 4096


def g3_tile(M, N, cus=256):
    """launch_gemm_g3's orientation rule -> (BM, BN): the one that needs fewer rounds of a block per CU; ties to the tall tile unless the
    wide one has fewer blocks and M < 256"""
    blocks = lambda bm, bn: -(-M // bm) * -(-N // bn)
    tall, wide = blocks(256, 128), blocks(128, 256)
    rt, rw = -(-tall // cus), -(-wide // cus)
    return (128, 256) if (rw < rt or (rw == rt and wide < tall and M < 256)) else (256, 128)


def g3_part_filled_block(M, ff):
    """the last pair-ordered column block of GEMM_SWIGLU holds fewer (gate, up) tile pairs than it has room for"""
    per = g3_tile(M, 2 * ff)[1] // 2
    return ff % per != 0


def g3_k_tiles(K):
    return -(-K // 64), K % 64 != 0


def attn_key_tiles(case):
    return -(-case.Tk // 64)


def attn_wholly_masked_tiles(case):
    """causal: some wave of a 64-query block (16 queries each) sees none of a key tile the block loads"""
    if not case.causal:
        return False
    for blk in range(0, case.Tq, 64):
        kmax = min(case.Tk, case.q_offset + min(case.Tq - 1, blk + 63) + 1)
        for w in range(4):
            rows = [r for r in range(blk + 16 * w, blk + 16 * w + 16) if r < case.Tq]
            if rows and any(j0 > case.q_offset + max(rows) for j0 in range(0, kmax, 64)):
                return True
    return False
