"""Inputs, references and the mirrored routing of the prefill GEMM op tests (tests/test_gemm_host.py checks them on the CPU,
tests/test_gpu_gemm.py feeds the same objects to dtk_op_gemm_ex).

A case holds the buffers of ONE GEMM call as the product makes it — A [M][lda] and W [N][ldw] with lda, ldw > K, bias / residual / C at
element offsets inside their buffers with their own row strides, the residual optionally C itself — and two references:

  mode "f64": A . W^T on the exact operand values in float64, then the kernel's bf16 rounding points (the Linear's output, the GELU, the
              gate, the gated product, the residual add).  A sliced-K call adds the slices' sums in slice order in fp32, as the kernels do.
  mode "f32": the same chain on the oracle's own float32 lines: oracle.ops.linear, torch's GELU (erf / tanh), torch's bf16 sigmoid.

Poison.  C starts as a quiet NaN with its own payload (in place: the [M][N] cells hold the residual), every input gap holds NaN: k >= K of
the rows of A and W, n >= N of the residual rows, the elements in front of the offsets.  A, residual and C have M rows exactly.  judge()
demands that every cell outside [M][N] keeps its bits, and that nothing behind the buffer was written (the op's guard bytes: a host-side
mutant hands judge() the cells it wrote behind the end).

Operand classes.
  grid    dense small integers in A and W (|a|, |w| <= 4): every fp32 partial sum is an integer below 2^24 in any order; bias and residual
          in eighths; the gate picked so that float64 sigmoid(gate) lies >= 2^-6 bf16 ulp from a rounding boundary.  Every non-GELU
          epilogue has ONE value: bit-equal to the float64 reference for every kernel, tile and slice count.
  gelu    one 1 per row of A (at a column that moves with the row; row 0's lies in the K tail), so a pre-activation is ONE weight + bias:
          an eighth plus a bias of a few 256ths with |weight + bias| <= 4, drawn per column from the values whose rounded pre-activation has a float64
          GELU >= 2^-6 ulp from a bf16 boundary (built, not filtered: no output is left out).  Bit-equal too; the pre-activations are NOT
          bf16 numbers, so rounding the Linear output first or not gives different results.
  order   sliced-K only: slices of +2^25, four separate 1s, -2^25 (times powers of two per row and column).  Every slice sum is exact in
          any order; added slice by slice the result is 4, in one chain the 1s vanish beside 2^25 and the result is 0.
  random  normal operands as in test_op_gemm, judged by bars.

Bars (none invented here).  grid / gelu / order: equality of bits.  random with one rounding (no epilogue, bias): test_op_gemm's rel-L2 <
1e-3, <= 2.01 bf16 ulps, < 5 % differing (prefill_rows_cases.SINGLE_*).  random chained outputs (GELU, residual, gate): min(test_op_
attention's 4.01 ulps / 2e-3, twice the distance of the two references, MEASURED_CHAIN_* below, asserted by the host test).

Shapes.  Nothing is larger than about 300 x 2100 x 600 except the deep K = 4304 and the two sliced "xcd" cases (512 x 1032 x 128 and
384 x 2056 x 128): k_gemm_g3<SL> has no tile option, it takes its orientation from the block counts, and more than 8 column tiles WITH more
than one row block need M >= 385 for the tall tile (below that the wide tile has fewer blocks and is chosen) and M > 256 with fewer wide
than tall blocks for the wide one.  They are K = 128 deep, so they cost less than the 257 x 1032 x 136 one-chain case.

route() mirrors launch_gemm_mfma / launch_gemm_sk_partials / launch_gemm_g3_sliced / launch_gemm_naive (csrc/kernels_batched.hip) and
returns the launchers' kernel record (csrc/kernels.h: GEMM_KCODE); branches() mirrors the alignment tests of the epilogues.  The coverage
claims of the host test are computed from them, and the GPU test asserts that the device's record equals route()."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from oracle.ops import bits_to_f32, f32_to_bits, linear, rb
from tests.gemv_b_cases import ulp_report
from tests.prefill_rows_cases import ATTN_RL2, ATTN_ULPS, SINGLE_FRAC, SINGLE_RL2, SINGLE_ULPS, r64

BIAS, GELU, RES, GATED, ERF, TANH, INPLACE, NAIVE, WT, SL, KS_SHIFT = 1, 2, 4, 8, 16, 32, 64, 256, 512, 1024, 12      # include/dtk.h
NAN_C, NAN_GAP, GUARD = 0x7FC9, 0x7FE9, 0xFFFF
GUARD_CELLS = 128                           # the op's 256 guard bytes
EPI = {"none": 0, "bias": BIAS, "erf": BIAS | ERF, "tanh": BIAS | TANH, "bias_res": BIAS | RES, "inplace": BIAS | RES | INPLACE,
       "gated": BIAS | RES | GATED | INPLACE, "res": RES, "erf_res": BIAS | ERF | RES}
MARGIN = 2.0 ** -6                          # of a bf16 ulp: how far a grid value stays from a rounding boundary

# float64 vs float32 reference over the random chained cases and REDRAWS redraws of each (tests/test_gemm_host.py asserts them): worst
# 2.25 ulps (257 x 129 x 328, bias + residual, a redraw: a flip of the Linear output in front of a residual add that cancels most of
# it), rel-L2 5.02e-5 (31 x 264 x 4304, 8 slices, in place).  Twice the ulps is beyond the cap, so that bar IS test_op_attention's 4.01;
# the rel-L2 bar is 1.0e-4, a twentieth of the cap.
MEASURED_CHAIN_ULPS, MEASURED_CHAIN_RL2 = 2.25, 5.02e-5
REDRAWS = 4
CHAIN_ULPS, CHAIN_RL2 = min(ATTN_ULPS, 2 * MEASURED_CHAIN_ULPS), min(ATTN_RL2, 2 * MEASURED_CHAIN_RL2)

MUTATIONS = ("bias_after_rounding", "linear_unrounded", "erf_tanh_swap", "gate_unrounded", "gate_on_residual", "residual_before_gelu",
             "k_tail_dropped", "k_tail_twice", "last_slice_dropped", "one_chain", "clamped_row_stored", "ldc_as_n", "ldr_as_ldc",
             "coltiles_above_8_dropped", "rows_swapped_in_tile")


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)))


def boundary_distance(y):
    """float64 tensor -> distance of every value from the nearest bf16 rounding boundary, in bf16 ulps of the value (0 counts as far)"""
    y = y.double()
    yb = r64(y)
    a = yb.abs()
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a))))
    ulp = torch.exp2(e - 7)
    pow2 = a == torch.exp2(e)
    up = yb.abs() + ulp / 2                                   # boundary away from zero
    dn = yb.abs() - torch.where(pow2, ulp / 4, ulp / 2)      # ... and towards it (half the spacing below a power of two)
    d = torch.minimum((y.abs() - up).abs(), (y.abs() - dn).abs()) / ulp
    return torch.where(a > 0, d, torch.full_like(d, 1.0))


def gelu64(v, kind):
    v = v.double()
    if kind == "erf":
        return 0.5 * v * (1 + torch.erf(v * 0.70710678118654752440))
    return 0.5 * v * (1 + torch.tanh(0.7978845608028654 * (v + 0.044715 * v * v * v)))


def gelu_distance(v, kind):
    """distance of GELU(v) from a bf16 rounding boundary in ulps, LESS what the fp32 formula itself can be off: 0.5 v (1 + erf(..)) forms
    1 + erf in fp32, whose absolute error (a few units of 2^-24: erff / tanhf and the add, 4 allowed here) is a fixed fraction of 1 — for
    v towards -4 the result is ~1e-4 and that error is a sizeable part of ITS ulp, so those pre-activations are not used"""
    y = gelu64(v, kind)
    yb = r64(y).abs()
    ulp = torch.exp2(torch.floor(torch.log2(torch.where(yb > 0, yb, torch.ones_like(yb)))) - 7)
    return boundary_distance(y) - 4 * 0.5 * v.double().abs() * 2.0 ** -24 / ulp


def sigmoid64(g):
    return 1 / (1 + torch.exp(-g.double()))


def pick_gate():
    """the grid's gate logit: an eighth whose float64 sigmoid is >= MARGIN from a rounding boundary and >= 0.2 ulp from a bf16 number
    (so that leaving the gate unrounded shows)"""
    for k in range(1, 33):
        g = torch.tensor(k / 8.0)
        s = sigmoid64(g)
        ulp = 2.0 ** (math.floor(math.log2(float(s))) - 7)
        if float(boundary_distance(s)) >= MARGIN and abs(float(s - r64(s))) >= 0.2 * ulp:
            return g
    raise AssertionError("no gate")


GATE_GRID = pick_gate()
GELU_BIAS = [k / 256.0 for k in (0, 2, -2, 3, 4, -5, 6, -7)]      # the columns' biases: with an eighth they are no bf16 number (except 0)
_GELU_ALLOWED = {}


def gelu_allowed(kind):
    """per bias of GELU_BIAS: the weights (eighths in [-4, 4]) whose pre-activation rounds to a value with a GELU >= MARGIN from a boundary"""
    if kind not in _GELU_ALLOWED:
        out = []
        w = torch.arange(-32, 33).double() / 8
        for b in GELU_BIAS:
            v = r64(w + b)
            out.append(w[(gelu_distance(v, kind) >= MARGIN) & ((w + b).abs() <= 4)].float())      # the pre-activation itself stays within [-4, 4]
        _GELU_ALLOWED[kind] = out
    return _GELU_ALLOWED[kind]


def slice_ranges(K, S):
    """the k ranges of the slices of a sliced-K role (kernels.h: sk_tiles_per_slice; the ragged tail belongs to the last slice)"""
    T = K // 64
    if S == 0:
        return [(0, K)]
    q = (T + S - 1) // S
    out = []
    for s in range(S):
        t0 = min(s * q, T)
        t1 = min(t0 + q, T)
        out.append((t0 * 64, K if s == S - 1 else t1 * 64))
    return out


class GemmCase:
    def __init__(self, tag, cls, M, N, K, epi, S=0, pat=(0, 8, 0, 0, 0), lda=None, ldw=None, contain=None, seed=0):
        self.tag, self.cls, self.M, self.N, self.K, self.epi, self.S, self.pat, self.contain, self.seed = tag, cls, M, N, K, epi, S, pat, contain, seed
        self.flags = EPI[epi]
        self.inplace = bool(self.flags & INPLACE)
        self.lda, self.ldw = lda or K + 8, ldw or K + 24
        self.ldc, self.c_off, self.b_off = N + pat[0], pat[2], pat[4]
        self.ldr, self.r_off = (self.ldc, self.c_off) if self.inplace else (N + pat[1], pat[3])
        self._args = dict(tag=tag, cls=cls, M=M, N=N, K=K, epi=epi, S=S, pat=pat, lda=lda, ldw=ldw, contain=contain)
        g = _gen(M, N, K, S, len(epi), sum(pat), seed, len(cls))
        if cls == "grid":
            self.A = torch.randint(-4, 5, (M, K), generator=g).float()
            self.W = torch.randint(-4, 5, (N, K), generator=g).float()
            self.bias = torch.randint(-32, 33, (N,), generator=g).float() / 8
            self.res = torch.randint(-32, 33, (M, N), generator=g).float() / 8
            self.gate = GATE_GRID.clone()
        elif cls == "gelu":
            kind = "erf" if self.flags & ERF else "tanh"
            allowed = gelu_allowed(kind)
            self.hot = [(K - 1 - 5 * m) % K for m in range(M)]
            self.A = torch.zeros(M, K)
            self.A[torch.arange(M), torch.tensor(self.hot)] = 1.0
            self.bias = torch.tensor([GELU_BIAS[n % len(GELU_BIAS)] for n in range(N)])
            self.W = torch.zeros(N, K)
            for n in range(N):
                a = allowed[n % len(GELU_BIAS)]
                self.W[n] = a[torch.randint(0, len(a), (K,), generator=g)]
            self.res, self.gate = torch.zeros(M, N), torch.tensor(0.0)
        elif cls == "order":
            am = torch.tensor([float(2 ** (m % 2)) for m in range(M)])
            wn = torch.tensor([(1.0, -1.0, 2.0)[n % 3] for n in range(N)])
            self.A, self.W = torch.zeros(M, K), torch.zeros(N, K)
            for s, (k0, k1) in enumerate(slice_ranges(K, S)):
                assert k1 - k0 >= 128
                if s % 3 == 1:
                    ks = [k0 + 32 * j for j in range(4)]
                    self.A[:, ks] = am[:, None]
                    self.W[:, ks] = wn[:, None]
                else:
                    self.A[:, k0:k0 + 64] = 1024.0 * am[:, None]
                    self.W[:, k0:k0 + 64] = (512.0 if s % 3 == 0 else -512.0) * wn[:, None]
            self.bias, self.res, self.gate = torch.zeros(N), torch.zeros(M, N), torch.tensor(0.0)
        else:
            self.A = rb(torch.randn(M, K, generator=g))
            self.W = rb(torch.randn(N, K, generator=g) * 0.05)
            self.bias = rb(torch.randn(N, generator=g) * 0.1)
            self.res = rb(torch.randn(M, N, generator=g))
            self.gate = rb(torch.randn((), generator=g) * 0.5)
        if contain == "a_nan":
            self.A[M - 1, 3 % K] = float("nan")
        elif contain == "w_nan":
            self.W[N - 1, K - 1] = float("nan")
        elif contain == "res_inf":
            self.res[M // 2, N // 2] = float("inf")

    def redraw(self, seed):
        return GemmCase(**self._args, seed=seed)

    @property
    def name(self):
        p = ".".join(str(x) for x in self.pat)
        return f"{self.cls}-{self.tag}-{self.M}x{self.N}x{self.K}-{self.epi}-S{self.S}-p{p}" + (f"-{self.contain}" if self.contain else "") + \
            (f"-seed{self.seed}" if self.seed else "")

    @property
    def kind(self):
        return "exact" if self.cls != "random" else ("single" if self.epi in ("none", "bias") else "chain")

    # ------------------------------------------------------------------------------------------ buffers
    def a_buffer(self):
        b = np.full((self.M, self.lda), NAN_GAP, dtype=np.uint16)
        b[:, :self.K] = f32_to_bits(self.A)
        return b.reshape(-1)

    def w_buffer(self):
        b = np.full((self.N, self.ldw), NAN_GAP, dtype=np.uint16)
        b[:, :self.K] = f32_to_bits(self.W)
        return b.reshape(-1)

    def bias_buffer(self):
        b = np.full(self.b_off + self.N, NAN_GAP, dtype=np.uint16)
        b[self.b_off:] = f32_to_bits(self.bias)
        return b

    def res_buffer(self):
        b = np.full(self.r_off + self.M * self.ldr, NAN_GAP, dtype=np.uint16)
        b[self.r_off:].reshape(self.M, self.ldr)[:, :self.N] = f32_to_bits(self.res)
        return b

    def gate_buffer(self):
        return f32_to_bits(self.gate.reshape(1))

    def cells(self, ld=None):
        ld = ld or self.ldc
        return (self.c_off + np.arange(self.M)[:, None] * ld + np.arange(self.N)[None, :]).reshape(-1)

    def initial(self):
        b = np.full(self.c_off + self.M * self.ldc, NAN_C, dtype=np.uint16)
        if self.inplace:
            b[self.cells()] = f32_to_bits(self.res).reshape(-1)
        return b

    def place(self, values):
        b = self.initial()
        b[self.cells()] = f32_to_bits(values.float().contiguous()).reshape(-1)
        return b

    # ------------------------------------------------------------------------------------------ references
    def accumulate(self, mode="f64", mutate=None):
        A, W, K = self.A, self.W, self.K
        seg = (lambda k0, k1: A[:, k0:k1].double() @ W[:, k0:k1].double().t()) if mode == "f64" else (lambda k0, k1: A[:, k0:k1] @ W[:, k0:k1].t())
        tail0 = (K // 64) * 64
        if mutate == "one_chain":           # every 32-wide k-step added to ONE fp32 accumulator
            acc = torch.zeros(self.M, self.N, dtype=torch.float64)
            for k0 in range(0, K, 32):
                acc = (acc + seg(k0, min(k0 + 32, K))).float().double()
            return acc
        ranges = slice_ranges(K, self.S)
        if mutate == "last_slice_dropped":
            ranges = ranges[:-1]
        sums = []
        for i, (k0, k1) in enumerate(ranges):
            if mutate == "k_tail_dropped":
                k1 = min(k1, tail0)
            s = seg(k0, max(k0, k1))
            if mutate == "k_tail_twice" and i == len(ranges) - 1:
                s = s + seg(tail0, K)
            sums.append(s)
        if len(sums) == 1:
            return sums[0]
        tot = sums[0].float()
        for s in sums[1:]:                  # fp32 adds in slice order (float64: of the exact slice sums, each add rounded once)
            tot = (tot.double() + s.float().double()).float() if mode == "f64" else tot + s
        return tot.double() if mode == "f64" else tot

    def res_values(self, mutate=None):
        if mutate == "ldr_as_ldc":
            buf = self.res_buffer()
            idx = (self.r_off + np.arange(self.M)[:, None] * self.ldc + np.arange(self.N)[None, :]) % buf.size
            return bits_to_f32(buf[idx.reshape(-1)]).reshape(self.M, self.N)
        return self.res

    def reference(self, mode="f64", mutate=None):
        f = self.flags
        if mode == "f32":
            assert mutate is None
            if self.S == 0:
                y = linear(self.A, self.W, self.bias if f & BIAS else None)
            else:
                acc = self.accumulate("f32")
                y = rb(acc + self.bias if f & BIAS else acc)
            if f & ERF:
                y = rb(torch.nn.functional.gelu(y))
            elif f & TANH:
                y = rb(torch.nn.functional.gelu(y, approximate="tanh"))
            if f & GATED:
                y = rb(torch.sigmoid(self.gate.to(torch.bfloat16)).float() * y)
            if f & RES:
                y = rb(self.res + y)
            return y
        acc = self.accumulate("f64", mutate)
        bias, res = self.bias.double(), self.res_values(mutate).double()
        if f & BIAS:
            v = r64(acc) + bias if mutate == "bias_after_rounding" else acc + bias
        else:
            v = acc
        if mutate != "linear_unrounded":
            v = r64(v)
        late_res = bool(f & RES)
        if mutate == "residual_before_gelu" and late_res:
            v, late_res = r64(res + v), False
        if f & (ERF | TANH):
            kind = "erf" if f & ERF else "tanh"
            if mutate == "erf_tanh_swap":
                kind = "tanh" if kind == "erf" else "erf"
            v = r64(gelu64(v, kind))
        if f & GATED:
            gs = sigmoid64(self.gate)
            if mutate != "gate_unrounded":
                gs = r64(gs)
            if mutate == "gate_on_residual":
                res = r64(gs * res)
            else:
                v = r64(gs * v)
        if late_res:
            v = r64(res + v)
        return v.float()

    def ref(self, mode="f64"):
        memo = self.__dict__.setdefault("_memo", {})
        if mode not in memo:
            memo[mode] = self.reference(mode)
        return memo[mode]

    def wrong(self, mutate):
        """the C buffer a kernel with this fault would leave (behind its end: the cells of the op's guard it wrote)"""
        M, N = self.M, self.N
        v = self.reference("f64", mutate)
        if mutate == "rows_swapped_in_tile":
            m, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
            v = v[torch.clamp(m // 16 * 16 + n % 16, max=M - 1), torch.clamp(n // 16 * 16 + m % 16, max=N - 1)]
        bits = f32_to_bits(v.float().contiguous())
        b = self.initial()
        if mutate == "ldc_as_n":
            b[self.cells(N)] = bits.reshape(-1)
        elif mutate == "coltiles_above_8_dropped":
            keep = 8 * self.xcd_width()
            b[self.cells().reshape(M, N)[:, :keep].reshape(-1)] = bits[:, :keep].reshape(-1)
        else:
            b[self.cells()] = bits.reshape(-1)
        if mutate == "clamped_row_stored":
            b = np.concatenate([b, np.full(GUARD_CELLS, GUARD, dtype=np.uint16)])
            at = self.c_off + M * self.ldc
            n = max(0, min(N, b.size - at))
            b[at:at + n] = bits[M - 1, :n]
        return b

    def xcd_width(self):
        """the widest tile of which N has more than 8"""
        return max([w for w in (32, 64, 128, 256) if self.N > 8 * w], default=0)

    def applies(self, m):
        f, exact = self.flags, self.kind == "exact"
        tail = self.K % 64 != 0
        if self.contain:
            return False
        return {"bias_after_rounding": bool(f & BIAS) and ((self.cls == "grid" and self.K >= 192 and self.M * self.N >= 1000) or self.epi == "bias" and self.cls == "random"),
                "linear_unrounded": self.cls == "gelu",
                "erf_tanh_swap": self.cls == "gelu",
                "gate_unrounded": bool(f & GATED) and self.cls == "grid",
                "gate_on_residual": bool(f & GATED),
                "residual_before_gelu": bool(f & RES) and bool(f & (ERF | TANH)),
                "k_tail_dropped": tail and self.cls != "order",
                "k_tail_twice": tail and self.cls != "order",
                "last_slice_dropped": self.S >= 2 and slice_ranges(self.K, self.S)[-1][1] > slice_ranges(self.K, self.S)[-1][0],
                "one_chain": self.cls == "order",
                "clamped_row_stored": True,
                "ldc_as_n": self.ldc != self.N and self.M > 1,
                "ldr_as_ldc": bool(f & RES) and not self.inplace and self.ldr != self.ldc and self.M > 1,
                "coltiles_above_8_dropped": self.xcd_width() > 0,
                "rows_swapped_in_tile": self.M * self.N > 1 and self.cls != "order"}[m]

    # ------------------------------------------------------------------------------------------ judging
    def judge(self, got):
        """got = the C buffer after the run (a host-side mutant: plus the guard cells it wrote).  Returns (ok, figures)."""
        got = np.asarray(got).reshape(-1)
        init = self.initial()
        fig = {"untouched": True, "contained": True, "exact": True, "single": (0.0, 0.0, 0.0), "chain": (0.0, 0.0)}
        if got.size > init.size:
            fig["untouched"] = bool((got[init.size:] == GUARD).all())
            got = got[:init.size]
        idx = self.cells()
        mask = np.zeros(init.size, dtype=bool)
        mask[idx] = True
        if not np.array_equal(got[~mask], init[~mask]):
            fig["untouched"] = False
        want = self.ref()
        g = got[idx]
        wnan = torch.isnan(want).reshape(-1).numpy()
        if wnan.any():                      # where the reference is NaN any NaN will do; everywhere else the cells are judged as usual
            fig["contained"] = bool(np.isnan(bits_to_f32(g[wnan]).numpy()).all())
        wb = f32_to_bits(want.contiguous()).reshape(-1)
        if self.kind == "exact":
            fig["exact"] = bool(np.array_equal(g[~wnan], wb[~wnan]))
        else:
            rep = ulp_report(bits_to_f32(g[~wnan]), bits_to_f32(wb[~wnan]))
            if self.kind == "single":
                fig["single"] = rep
            else:
                fig["chain"] = rep[1:]
        fr, u, r = fig["single"]
        ok = fig["untouched"] and fig["contained"] and fig["exact"] and fr < SINGLE_FRAC and u <= SINGLE_ULPS and r < SINGLE_RL2 and \
            fig["chain"][0] <= CHAIN_ULPS and fig["chain"][1] < CHAIN_RL2
        return bool(ok), fig

    def reference_distance(self):
        """(ulps, rel-L2) between the float32 and the float64 reference of a chained output"""
        return ulp_report(self.ref("f32"), self.ref())[1:]


# ---------------------------------------------------------------------------------------------------- the case lists
PAT = [(0, 8, 0, 0, 0), (8, 0, 0, 0, 4), (4, 8, 0, 4, 0), (2, 4, 0, 0, 2), (8, 2, 4, 0, 1), (0, 8, 2, 1, 0), (8, 16, 1, 2, 0), (8, 4, 0, 2, 0)]
GRID_EPIS = ("none", "bias", "bias_res", "inplace", "gated", "res")
K_AXIS = (8, 40, 64, 72, 128, 136, 192, 200, 256, 328)
M_AXIS = (1, 31, 32, 33, 63, 65, 127, 129, 255, 257)
N_AXIS = (1, 7, 30, 36, 31, 33, 63, 65, 127, 129)
XCD_SHAPES = ((65, 264), (129, 520), (129, 1032), (257, 1032), (129, 2056))       # more than 8 column tiles AND more than one row block per tile shape
SK_SHAPES = {128: (33, 36), 200: (65, 136), 576: (129, 260), 4304: (31, 264)}
_CACHE = {}


def one_chain_cases():
    if "one" in _CACHE:
        return _CACHE["one"]
    cs = []
    for i, (M, N, K) in enumerate(zip(M_AXIS, N_AXIS, K_AXIS)):                       # the K axis against the M and N axes
        cs.append(GemmCase("axis", "grid", M, N, K, GRID_EPIS[i % 6], pat=PAT[i % 8]))
    for i, (M, N) in enumerate(((33, 255), (31, 257), (1, 264))):                    # the wide tiles' edges, and M = 1 over 9 column tiles
        cs.append(GemmCase("edge", "grid", M, N, 136, GRID_EPIS[(i + 2) % 6], pat=PAT[(i + 3) % 8]))
    for i, (M, N) in enumerate(XCD_SHAPES):
        cs.append(GemmCase("xcd", "grid", M, N, 136, GRID_EPIS[(i + 1) % 6], pat=PAT[(2 * i + 1) % 8]))
    cs.append(GemmCase("deep", "grid", 65, 40, 4304, "bias_res", pat=PAT[1]))
    for epi in ("bias_res", "inplace", "gated"):                                    # every alignment pattern at an N that may take the LDS epilogue
        for p in PAT:
            cs.append(GemmCase("align", "grid", 33, 136, 136, epi, pat=p))
    cs.append(GemmCase("align", "grid", 33, 36, 136, "bias_res", pat=PAT[0]))        # N % 8 != 0 with everything else aligned
    cs.append(GemmCase("align", "grid", 33, 30, 136, "bias_res", pat=PAT[0]))        # N % 4 != 0
    cs.append(GemmCase("align", "grid", 257, 136, 200, "inplace", pat=PAT[1]))       # the LDS epilogue over two row blocks of the tall tile
    # the product's own calls (dtk_api.hip): the patch embedding (K = lda = ldw = the padded 592, pos_embed as residual with its own stride),
    # a ViT block's in-place residual, the image query at M = 1 and the pooling head at M = B
    cs.append(GemmCase("patch-embed", "grid", 36, 144, 592, "bias_res", pat=(8, 0, 0, 0, 0), lda=592, ldw=592))
    cs.append(GemmCase("vit-inplace", "grid", 65, 144, 144, "inplace", pat=(0, 0, 0, 0, 0), lda=144, ldw=144))
    cs.append(GemmCase("image-query", "grid", 1, 144, 144, "bias", pat=(0, 0, 0, 0, 0), lda=144, ldw=144))
    cs.append(GemmCase("pool-head", "grid", 3, 144, 144, "bias", pat=(0, 0, 0, 0, 0), lda=144, ldw=144))
    for kind in ("erf", "tanh"):
        for i, (M, N, K) in enumerate(((31, 33, 40), (65, 36, 72), (33, 136, 136), (129, 65, 200))):
            cs.append(GemmCase("gelu", "gelu", M, N, K, kind, pat=PAT[(i + (kind == "tanh")) % 8]))
    for M, N, K, epi, contain in ((33, 36, 136, "bias_res", "a_nan"), (33, 36, 136, "bias", "w_nan"), (33, 36, 136, "bias_res", "res_inf"),
                                  (65, 136, 200, "bias", "a_nan"), (65, 136, 200, "inplace", "w_nan"), (257, 136, 72, "inplace", "res_inf")):
        cs.append(GemmCase("contain", "grid", M, N, K, epi, pat=PAT[0] if N == 36 else PAT[1], contain=contain))
    for i, (M, N, K, epi) in enumerate(((33, 36, 72, "none"), (65, 33, 136, "bias"), (129, 65, 200, "erf"), (127, 63, 192, "tanh"), (257, 129, 328, "bias_res"),
                                        (63, 136, 128, "inplace"), (33, 136, 136, "gated"), (31, 257, 136, "res"), (65, 40, 4304, "bias"),
                                        (129, 264, 136, "erf_res"), (36, 144, 592, "erf_res"), (1, 144, 40, "tanh"))):
        cs.append(GemmCase("rand", "random", M, N, K, epi, pat=PAT[i % 8]))
    _CACHE["one"] = cs
    return cs


def sliced_cases():
    if "sk" in _CACHE:
        return _CACHE["sk"]
    cs = []
    for ki, (K, (M, N)) in enumerate(SK_SHAPES.items()):
        for S in range(1, 9):
            cs.append(GemmCase("sk", "grid", M, N, K, GRID_EPIS[(S + ki) % 6], S=S, pat=PAT[(S + 2 * ki) % 8]))
    # k_gemm_g3<SL> takes its orientation from the block counts: these two give each one more than 8 column tiles and several row blocks
    # (the only cases beyond ~300 rows: see "Shapes" in the module docstring)
    cs.append(GemmCase("xcd", "grid", 512, 1032, 128, "bias_res", S=2, pat=PAT[1]))
    cs.append(GemmCase("xcd", "grid", 384, 2056, 128, "inplace", S=3, pat=PAT[0]))
    cs.append(GemmCase("order", "order", 33, 36, 384, "none", S=3, pat=PAT[0]))
    cs.append(GemmCase("order", "order", 65, 136, 768, "none", S=6, pat=PAT[1]))
    for i, (M, N, K, S, epi) in enumerate(((65, 136, 200, 2, "bias_res"), (129, 260, 576, 5, "none"), (31, 264, 4304, 8, "inplace"), (33, 36, 128, 3, "bias"))):
        cs.append(GemmCase("rand", "random", M, N, K, epi, S=S, pat=PAT[(i + 1) % 8]))
    _CACHE["sk"] = cs
    return cs


def all_cases():
    return one_chain_cases() + sliced_cases()


# ---------------------------------------------------------------------------------------------------- variants and the mirrored routing
DEFAULTS = dict(gemm_impl=3, gemm_tile=0, gemm_stages=3, gemm_bk=64, gemm_g3_min_blocks=128, gemm_glds_min_tiles=160, gemm_g3_tile=0,
                gemm_epi_direct=0, gemm_wt=1, gemm_sk_tile=2)
Variant = namedtuple("Variant", "name family opts flags")
CUS = 256                                                                            # MI355X


def variants(family):
    if family.startswith("mfma-t"):
        t = int(family[-1])
        out = [Variant(f"{family}-D{D}", family, dict(gemm_impl=0, gemm_tile=t, gemm_stages=D), 0) for D in (1, 2, 3, 4)]
        if t == 1:
            out += [Variant(f"{family}-D{D}-bk128", family, dict(gemm_impl=0, gemm_tile=1, gemm_stages=D, gemm_bk=128), 0) for D in (1, 2, 3, 4)]
        return out
    if family == "default":
        return [Variant("default", family, {}, 0)]
    if family == "glds":
        return [Variant("glds", family, dict(gemm_impl=2, gemm_glds_min_tiles=1), 0)]
    if family in ("g3-tall", "g3-wide"):
        return [Variant(f"{family}-{'wt' if wt else 'rm'}-{'direct' if d else 'lds'}", family,
                        dict(gemm_impl=4, gemm_g3_min_blocks=1, gemm_g3_tile=1 if family == "g3-tall" else 2, gemm_epi_direct=d), WT if wt else 0)
                for wt in (0, 1) for d in (0, 1)]
    if family == "sk":
        return [Variant(f"sk-{'wide' if t else 'tall'}-{'wt' if wt else 'rm'}-{'direct' if d else 'lds'}", family, dict(gemm_sk_tile=t, gemm_epi_direct=d), WT if wt else 0)
                for t in (0, 1) for wt in (0, 1) for d in (0, 1)]
    if family == "sl":
        return [Variant(f"sl-{'wt' if wt else 'rm'}-{'direct' if d else 'lds'}", family, dict(gemm_epi_direct=d), SL | (WT if wt else 0)) for wt in (0, 1) for d in (0, 1)]
    if family == "naive":
        return [Variant("naive", family, {}, NAIVE)]
    raise KeyError(family)


ONE_CHAIN_FAMILIES = ("mfma-t1", "mfma-t2", "mfma-t3", "mfma-t4", "mfma-t5", "default", "glds", "g3-tall", "g3-wide", "naive")
SLICED_FAMILIES = ("sk", "sl", "naive")
MFMA_ORDER = ("mfma-t1", "mfma-t2", "mfma-t3", "mfma-t4", "mfma-t5", "default", "glds", "g3-tall", "g3-wide", "sk", "sl")      # the families that promise ONE k order


def anchor(c):
    """the fixed kernel whose bits every one-k-order kernel must reproduce on a random case: k_gemm_mfma 64 x 64 with 3 register stages
    for a one-chain call, the tall row-major sliced-K pair through LDS for a sliced one"""
    return variants("sk")[0] if c.S else variants("mfma-t1")[2]


def cases_of(family):
    if family == "sl":
        return [c for c in sliced_cases() if c.S >= 2]
    if family == "sk":
        return sliced_cases()
    if family == "naive":
        return all_cases()
    return one_chain_cases()


def kcode(family, tile=0, stages=0, bk128=0, wt=0, epi=0, slices=0):
    return family | tile << 4 | stages << 8 | bk128 << 12 | wt << 13 | epi << 14 | slices << 16


def blocks(M, N, bm, bn):
    return ((M + bm - 1) // bm) * ((N + bn - 1) // bn)


def g3_epi(c, o, sk):
    lds = not o["gemm_epi_direct"] and c.N % 8 == 0 and (sk or (c.ldc % 8 == 0 and (2 * c.c_off) % 16 == 0))
    return 1 if lds else 2


def route(c, v):
    """the launchers' record (csrc/kernels.h: GEMM_KCODE) of the kernel this call ends at; A and W are 16-byte aligned with lda, ldw % 8 == 0"""
    o = dict(DEFAULTS, **v.opts)
    M, N, K, S = c.M, c.N, c.K, c.S
    wt = 1 if (v.flags & WT) and o["gemm_wt"] else 0
    if v.flags & NAIVE:
        return kcode(6, slices=S if S > 1 else 0)
    if S and v.flags & SL:
        wide = blocks(M, N, 128, 256) < blocks(M, N, 256, 128)
        return kcode(5, 7 if wide else 6, wt=wt, epi=g3_epi(c, o, False), slices=S)
    if S:
        wide = M <= 128 if o["gemm_sk_tile"] == 2 else o["gemm_sk_tile"] == 1
        return kcode(4, 7 if wide else 6, wt=wt, epi=g3_epi(c, o, True), slices=S)
    over = o["gemm_tile"]
    if o["gemm_impl"] in (3, 4) and not over and K >= 128:
        tall, wide = blocks(M, N, 256, 128), blocks(M, N, 128, 256)
        rt, rw = (tall + CUS - 1) // CUS, (wide + CUS - 1) // CUS
        use_wide = o["gemm_g3_tile"] == 2 if o["gemm_g3_tile"] else (rw < rt or (rw == rt and wide < tall and M < 256))
        if (wide if use_wide else tall) >= o["gemm_g3_min_blocks"]:
            return kcode(3, 7 if use_wide else 6, wt=wt, epi=g3_epi(c, o, False))
    if (o["gemm_impl"] == 2 or (o["gemm_impl"] in (3, 4) and M >= 1024)) and not over and K >= 64 and blocks(M, N, 128, 128) >= o["gemm_glds_min_tiles"]:
        return kcode(2, 3)
    tile = over or (1 if blocks(M, N, 64, 64) >= 512 else (4 if blocks(M, N, 64, 32) >= 512 else 5))
    D, bk128 = o["gemm_stages"], int(tile == 1 and o["gemm_bk"] == 128)
    return kcode(1, tile, D if D in (1, 2) or (D == 4 and not bk128) else 3, bk128)


def branches(c, v):
    """which alignment branches of the routed kernel's epilogue (and of k_sk_reduce) this call takes"""
    code = route(c, v)
    fam, epi = code & 15, (code >> 14) & 3
    f = c.flags
    cp, rp, bp = 2 * c.c_off, 2 * c.r_off, 2 * c.b_off                 # byte offsets of the pointers from a 256-byte aligned base
    out = set()
    if fam in (1, 2):
        out.add("tiles")
    if fam == 4:
        out.add("sk_lds" if epi == 1 else "sk_direct")
        out.add("red_vec" if c.ldc % 4 == 0 and cp % 8 == 0 else "red_novec")
        if f & RES:
            out.add("red_rvec" if c.ldr % 4 == 0 and rp % 8 == 0 else "red_rscalar")
        if f & BIAS:
            out.add("red_bvec" if bp % 8 == 0 else "red_bscalar")
    if fam in (3, 5) and epi == 1:
        out.add("lds")
        if f & BIAS:
            out.add("lds_bias16" if bp % 16 == 0 else "lds_bias_scalar")
        if f & RES:
            out.add("lds_rvec" if c.ldr % 8 == 0 and rp % 16 == 0 else "lds_rscalar")
    if fam in (3, 5) and epi == 2:
        o = dict(DEFAULTS, **v.opts)
        out.add("direct_forced" if o["gemm_epi_direct"] else ("direct_n8" if c.N % 8 else "direct_ldc8"))
        nvec = c.N % 4 == 0
        out.add("vec" if c.ldc % 4 == 0 and cp % 8 == 0 else "novec")
        out.add("nvec" if nvec else "scalar_cols")
        if f & RES:
            out.add("rvec" if nvec and c.ldr % 4 == 0 and rp % 8 == 0 else "rscalar")
        if f & BIAS:
            out.add("bvec" if nvec and bp % 8 == 0 else "bscalar")
    return out


def instantiations():
    """every GEMM kernel instantiation the launchers compile, as records without the epilogue and slice fields"""
    out = {kcode(1, t, D) for t in (1, 2, 3, 4, 5) for D in (1, 2, 3, 4)} | {kcode(1, 1, D, 1) for D in (1, 2, 3)} | {kcode(2, 3)}
    out |= {kcode(fam, t, wt=wt) for fam in (3, 4, 5) for t in (6, 7) for wt in (0, 1)} | {kcode(6)}
    return out


def strip(code):
    return code & 0x3FFF
