// kernels_decode.hip — the tokens/sec kernel set: one decoded token = 5 kernels per
// LLaMA layer + lm_head + sampler, all HBM-bound weight streaming (SURVEY §8 rows
// a·D-step, a·H, a·S).  Numerics follow HF modeling_llama.py in bf16: every tensor HF
// materialises is rounded to bf16 at the same point, dot products accumulate in fp32.
//
// GEMV family (k_gemv): y = W . x with W [N][K] bf16 streamed exactly once with
// non-temporal 16-byte loads straight into VGPRs (no LDS round trip: each weight byte is
// used by one wave once), x staged in LDS (bf16) by a fused prologue:
//   PRO_RMSNORM  x = rmsnorm(residual)            (input_layernorm / post_attention / final norm)
//   PRO_ATTN     x = combine of the split-K attention partials (flash-decode reduction)
//   PRO_COPY     x = activation vector
// and a fused epilogue on the wave-reduced sums:
//   EPI_QKV      RoPE (rotate-half) on q,k pairs, q -> scratch, k,v -> KV cache at pos
//   EPI_SWIGLU   silu(gate)*up
//   EPI_RESID    residual += y
//   EPI_LOGITS   fp32 logits
// Each wave owns NR weight rows for the full K, lanes stride K in 16-byte chunks
// (64 lanes x 16 B = 1 KiB per row per load instruction), two register stages so the
// next stage's loads are in flight while the current one is consumed by v_dot2c_f32_bf16.
#include <cstdlib>
#include <cstring>
#include "kernels.h"
#include "gemv_inl.h"
#include "sample_inl.h"

// Epilogue of one output unit (one lane per wave): `a0` is the fp32 dot product of the unit's row (paired epilogues:
// a0 / a1 = the two rows of the pair: RoPE partners i, i + HD/2 or gate, up).  HD = head dim (EPI_QKV): 128, or 64 (TinyLlama).  Same HF rounding points as the reference.
// `pre0` / `pre1`: operands the epilogue needs from memory, loaded at kernel start by the lane that runs it (EPI_RESID: the
// residual value y[u]; EPI_QKV: cos / sin of (pos, i)) — a dependent load in the epilogue was ~1 us of exposed latency at
// the very end of every wave; `pos` likewise (read once at kernel start).
template <int EPI, bool F8, int HD = 128>
__device__ __forceinline__ void gemv_epilogue(const GemvArgs& a, int u, float a0, float a1, float pre0, float pre1, int pos) {
    constexpr int HD2 = HD / 2, HSH = HD == 128 ? 6 : 5;   // u >> HSH = head block of unit u
    static_assert(HD == 128 || HD == 64, "head dim 128 or 64");
    if (F8) {  // per-output-channel power-of-two scale (exact)
      if (EPI == EPI_QKV) {
        const int r0 = (u >> HSH) * HD + (u & (HD2 - 1));
        a0 *= a.wscale[r0];
        a1 *= a.wscale[r0 + HD2];
      } else if (EPI == EPI_SWIGLU) {
        a0 *= a.wscale[u];
        a1 *= a.wscale[a.ff + u];
      } else {
        a0 *= a.wscale[u];
      }
    }
    if (EPI == EPI_STORE) {
      a.y[u] = f2bf(a0);
    } else if (EPI == EPI_RESID) {
      // HF: hidden = residual + proj(x); proj output is a bf16 tensor
      a.y[u] = f2bf(pre0 + rbf(a0));
    } else if (EPI == EPI_LOGITS) {
      a.logits[u] = rbf(a0);  // lm_head output is bf16, then .float()
    } else if (EPI == EPI_SWIGLU) {
      const float gte = rbf(a0);
      const float up = rbf(a1);
      const float sl = rbf(gte / (1.f + expf(-gte)));
      a.y[u] = f2bf(sl * up);
    } else if (EPI == EPI_QKV) {
      const int hb = u >> HSH, i = u & (HD2 - 1);
      const int sec = hb < a.H ? 0 : (hb < a.H + a.KVH ? 1 : 2);
      const int head = sec == 0 ? hb : (sec == 1 ? hb - a.H : hb - a.H - a.KVH);
      const float x1 = rbf(a0);      // dim i
      const float x2 = rbf(a1);  // dim i + HD/2
      if (sec == 2) {
        bf16_t* dst = a.vcache + ((size_t)head * a.T_max + pos) * HD;
        dst[i] = f2bf(x1);
        dst[i + HD2] = f2bf(x2);
      } else {
        // HF apply_rotary_pos_emb: q*cos + rotate_half(q)*sin, every product a bf16 tensor
        const float c = pre0, s = pre1;
        const float o1 = rbf(rbf(x1 * c) + rbf(-x2 * s));
        const float o2 = rbf(rbf(x2 * c) + rbf(x1 * s));
        bf16_t* dst = (sec == 0) ? (a.q_out + head * HD)
                                 : (a.kcache + ((size_t)head * a.T_max + pos) * HD);
        dst[i] = f2bf(o1);
        dst[i + HD2] = f2bf(o2);
      }
    }
}

// R = output units per wave-chunk; paired epilogues (QKV, SWIGLU) stream 2 rows per unit.
// WAVES = waves per block.  PERSIST: grid-stride over chunks (chunk c -> block c % grid,
// wave (c / grid) % WAVES) so a grid sized to the machine covers any N with <= 1 chunk of
// imbalance per wave; otherwise one chunk per wave and the grid covers N.
// KS > 1: split-K over KS waves of the block — the k-groups of a row (pair) are dealt round-robin to KS waves, whose partial
// sums meet in LDS in a fixed order (deterministic).  For the N = d roles (o_proj, down: only d rows) this puts KS times the
// waves, hence loads, in flight per row; the block then owns WAVES / KS row-chunks.
// HD: head dim of the EPI_QKV rows / the PRO_ATTN partials (128, or 64: a unit is the pair (i, i+32), a head 8 chunks of x).
// F4: MXFP4 rows (a.W4 codes, a.S4 block scales; gemv_inl.h): a chunk = one 32-weight block, x swizzled in LDS (f4_xswz) and
// zero-padded to whole blocks, no row scale in the epilogue.  Every F4 branch is compile-time: the bf16 / fp8 code is unchanged.
// W13: the 13-bit planes of bf16 rows (a.Wp rows, a.Wh row bytes; w13.h, gemv_inl.h): the operands rebuilt in registers are the bf16
// row's bits and the fold order is gemv_fma's, so the sums are the bf16 kernel's; x lies linearly in LDS; U is a multiple of 4.  Every
// W13 branch is compile-time as well.  Rows whose byte a.Wh has W13_ZROW hold a zero code: under PRO_RMSNORM a wave decodes its row
// group by the general rule if any of its NR rows has the bit and by the short one otherwise (gemv_inl.h: dot8_w13<NZ>; wave-uniform,
// the same bits); the other prologues' roles (down, o_proj) gained nothing from the short decode and keep the general one alone.
// FW: PRO_RMSNORM folds the sum of squares per thread, per wave and over the waves, so `inv` depends on how many threads fold.  The
// first FW x 64 threads of the block fold exactly as a block of FW waves does (the same chunks per thread in the same order, in both
// forms of the prologue, whose choice follows FW as well), so a kernel of any block size gives the bits of the FW-wave kernel.  FW = WAVES
// is the code without the parameter.
template <int PRO, int EPI, int R, int U, int WAVES, bool PERSIST, bool F8 = false, int KS = 1, int HD = 128, bool F4 = false, bool W13 = false, int FW = WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_gemv(GemvArgs a) {
  static_assert(!(F4 && F8) && !(W13 && (F4 || F8)), "one weight format");
  static_assert(FW >= 1 && FW <= WAVES, "the folding threads are the block's first");
  constexpr int FT = FW * 64;                  // PRO_RMSNORM: threads that fold the sum of squares
  constexpr bool FALL = FW == WAVES;           // ... all of the block
  constexpr bool PAIRED = (EPI == EPI_QKV) || (EPI == EPI_SWIGLU);
  constexpr int NR = PAIRED ? 2 * R : R;
  constexpr int THREADS = WAVES * 64;
  constexpr int RW = WAVES / KS;               // row-chunks (of R units) per block
  constexpr int HD2 = HD / 2, HC = HD / 8;     // RoPE pair distance; 16-byte chunks of x per head
  constexpr int HSH = HD == 128 ? 6 : 5, CSH = HSH - 2;   // log2(HD2), log2(HC)
  static_assert(HD == 128 || HD == 64, "head dim 128 or 64");
  static_assert(WAVES % KS == 0 && (KS == 1 || !PERSIST), "split-K variants are not persistent");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u32x4* xs = reinterpret_cast<u32x4*>(smem);
  const int K8 = a.K >> 3;                     // 16-byte chunks of x (bf16)
  const int KC = F4 ? ((a.K + 31) >> 5) : (F8 ? (a.K >> 4) : K8);         // 16-byte chunks of one weight row
  const size_t row_bytes = W13 ? w13_row_bytes(a.K) : (F4 ? (size_t)KC * 16 : (F8 ? (size_t)a.K : (size_t)a.K * 2));
  const unsigned char* Wb = reinterpret_cast<const unsigned char*>(W13 ? (const void*)a.Wp : (F4 ? (const void*)a.W4 : (F8 ? (const void*)a.W8 : (const void*)a.W)));
  const int J2 = W13 ? w13_units(a.K) : 0, n13 = W13 ? (int)w13_n_off(a.K) : 0, s13 = W13 ? (int)w13_s_off(a.K) : 0;   // W13: units of a row, plane offsets
  float* red = reinterpret_cast<float*>(smem + (size_t)(F4 ? f4_xrows(KC) : K8) * 16);  // WAVES floats of scratch
#define XI(c) (F4 ? f4_xswz(c) : (c))          // where 16-byte piece c of x lies in LDS

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int rw = KS > 1 ? wave / KS : wave;    // which row-chunk of the block
  const int ks = KS > 1 ? wave % KS : 0;       // which share of K

  int n_units;
  if (EPI == EPI_QKV) n_units = (a.N >> 1);
  else if (EPI == EPI_SWIGLU) n_units = a.ff;
  else n_units = a.N;
  const int chunk_stride = PERSIST ? (int)gridDim.x * WAVES : 0;
  int chunk = PERSIST ? (int)blockIdx.x + (int)gridDim.x * wave : (int)blockIdx.x * RW + rw;
  int unit0 = chunk * R;

  const u32x4* rows[NR];
  const uint8_t* srows[NR];                    // F4: the rows' block scales
  uint32_t lo4[NR];                            // W13: the rows' decode base lo in every byte
  bool zrow = false;                           // W13: one of the wave's rows holds a zero code (wave-uniform)
  auto set_rows = [&](int u0) {
    unsigned zb = 0;                           // W13: the row bytes of the group, or-ed
#pragma unroll
    for (int j = 0; j < R; ++j) {
      int u = u0 + j;
      if (u >= n_units) u = n_units - 1;  // clamped: inactive tails never fault
      int r0, r1 = 0;
      if (EPI == EPI_QKV) {   // unit = RoPE pair (i, i+HD/2) of head block hb over [H q | KVH k | KVH v]
        r0 = (u >> HSH) * HD + (u & (HD2 - 1));
        r1 = r0 + HD2;
      } else if (EPI == EPI_SWIGLU) {
        r0 = u;
        r1 = a.ff + u;
      } else {
        r0 = u;
      }
      if (PAIRED) {
        rows[2 * j] = reinterpret_cast<const u32x4*>(Wb + (size_t)r0 * row_bytes);
        rows[2 * j + 1] = reinterpret_cast<const u32x4*>(Wb + (size_t)r1 * row_bytes);
      } else {
        rows[j] = reinterpret_cast<const u32x4*>(Wb + (size_t)r0 * row_bytes);
      }
      if (F4) {
        if (PAIRED) { srows[2 * j] = a.S4 + (size_t)r0 * KC; srows[2 * j + 1] = a.S4 + (size_t)r1 * KC; }
        else srows[j] = a.S4 + (size_t)r0 * KC;
      }
      if (W13) {
        const unsigned b0 = a.Wh[r0], b1 = PAIRED ? a.Wh[r1] : 0u;
        if (PAIRED) { lo4[2 * j] = (uint32_t)w13_lo(b0) * 0x01010101u; lo4[2 * j + 1] = (uint32_t)w13_lo(b1) * 0x01010101u; }
        else lo4[j] = (uint32_t)w13_lo(b0) * 0x01010101u;
        zb |= b0 | b1;
      }
    }
    if (W13 && PRO == PRO_RMSNORM) zrow = (__builtin_amdgcn_readfirstlane((int)zb) & W13_ZROW) != 0;   // every lane of the wave read the same bytes
  };
  set_rows(unit0);

  const int iters = (KC + 63) >> 6;
  const int Gall = (iters + U - 1) / U;
  const int G = KS > 1 ? (Gall - ks + KS - 1) / KS : Gall;    // k-groups of this wave: ks, ks + KS, ...
#define GIDX(g) (KS > 1 ? ks + KS * (g) : (g))
  u32x4 wa[NR][U], wb[NR][U];
  unsigned sa[NR][U], sb[NR][U];               // F4: the stages' block scales
  constexpr int UW = W13 ? U : 4;              // W13: the stages' planes (the other formats leave them unused)
  u32x4 lwa[NR][UW / 2], lwb[NR][UW / 2];
  u32x2 nwa[NR][UW / 2], nwb[NR][UW / 2];
  uint32_t zwa[NR][UW / 4], zwb[NR][UW / 4];
  float acc[NR];
#define GLOAD(w, sc, g) do { if (W13) gemv_load_w13<NR, UW>(l##w, n##w, z##w, rows, (g), lane, J2, n13, s13); else if (F4) gemv_load_f4<NR, U>(w, sc, rows, srows, (g), lane, KC); else gemv_load<NR, U>(w, rows, (g), lane, KC); } while (0)
#define GFMA(w, sc, g) do { if (W13) gemv_fma_w13<NR, UW, NZ>(acc, l##w, n##w, z##w, lo4, xs, (g), lane, K8); else if (F4) gemv_fma_f4<NR, U>(acc, w, sc, xs, (g), lane, KC); else if (F8) gemv_fma_f8<NR, U>(acc, w, xs, (g), lane, KC); else gemv_fma<NR, U>(acc, w, xs, (g), lane, KC); } while (0)

  // first stage of weights goes in flight before the prologue touches x
  if (G > 0) GLOAD(wa, sa, GIDX(0));

  // operands of the epilogue (see gemv_epilogue): issued now, consumed after the last weight chunk
  float pre0[R], pre1[R];
  int pos = 0;
  if (EPI == EPI_QKV) pos = a.st->pos;
  auto prefetch_epilogue = [&](int u0) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      pre0[j] = 0.f; pre1[j] = 0.f;
      if (lane == 0 && ks == 0) {
        int u = u0 + j;
        if (u >= n_units) u = n_units - 1;
        if (EPI == EPI_RESID) pre0[j] = bf2f(a.y[u]);
        if (EPI == EPI_QKV) {
          pre0[j] = bf2f(a.rope_cos[(size_t)pos * HD2 + (u & (HD2 - 1))]);
          pre1[j] = bf2f(a.rope_sin[(size_t)pos * HD2 + (u & (HD2 - 1))]);
        }
      }
    }
  };
  if (EPI == EPI_RESID || EPI == EPI_QKV) prefetch_epilogue(unit0);

  // ---- prologue: build the bf16 input vector in LDS
  if (PRO == PRO_COPY) {
    const u32x4* x4 = reinterpret_cast<const u32x4*>(a.x);
    for (int c = tid; c < K8; c += THREADS) xs[XI(c)] = x4[c];
  } else if (PRO == PRO_RMSNORM) {
    const u32x4* x4 = reinterpret_cast<const u32x4*>(a.x);
    const u32x4* w4 = reinterpret_cast<const u32x4*>(a.norm_w);
    if (K8 <= 2 * FT) {
      // x and the norm weight in ONE memory round trip, kept in registers across the block reduction (the two-pass form
      // re-read x after the barrier: a second dependent L1 / L2 trip in front of every RMSNorm GEMV).  FW < WAVES: the folding
      // threads hold all of x; the others only meet them at the barriers.
      const int c0 = tid, c1 = tid + FT;
      const bool h0 = (FALL || tid < FT) && c0 < K8, h1 = (FALL || tid < FT) && c1 < K8;
      const u32x4 zz = {0u, 0u, 0u, 0u};
      const u32x4 v0 = h0 ? x4[c0] : zz, v1 = h1 ? x4[c1] : zz;
      const u32x4 g0 = h0 ? w4[c0] : zz, g1 = h1 ? w4[c1] : zz;
      float ss = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float lo = pk_lo(v0[e]), hi = pk_hi(v0[e]);
        ss += lo * lo;
        ss += hi * hi;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float lo = pk_lo(v1[e]), hi = pk_hi(v1[e]);
        ss += lo * lo;
        ss += hi * hi;
      }
      ss = wave_sum(ss);
      if (lane == 0) red[wave] = ss;
      __syncthreads();
      float tot = 0.f;
#pragma unroll
      for (int w = 0; w < FW; ++w) tot += red[w];
      const float inv = rsqrtf(tot / (float)a.K + a.eps);
      u32x4 o0, o1;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // HF LlamaRMSNorm: weight * (x * rsqrt(var+eps)).to(bf16)
        o0[e] = pack2(pk_lo(g0[e]) * rbf(pk_lo(v0[e]) * inv), pk_hi(g0[e]) * rbf(pk_hi(v0[e]) * inv));
        o1[e] = pack2(pk_lo(g1[e]) * rbf(pk_lo(v1[e]) * inv), pk_hi(g1[e]) * rbf(pk_hi(v1[e]) * inv));
      }
      if (h0) xs[XI(c0)] = o0;
      if (h1) xs[XI(c1)] = o1;
    } else {
      float ss = 0.f;
      for (int c = (FALL || tid < FT) ? tid : K8; c < K8; c += FT) {   // FW < WAVES: only the folding threads sum; all normalise below
        const u32x4 v = x4[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float lo = pk_lo(v[e]), hi = pk_hi(v[e]);
          ss += lo * lo;
          ss += hi * hi;
        }
      }
      ss = wave_sum(ss);
      if (lane == 0) red[wave] = ss;
      __syncthreads();
      float tot = 0.f;
#pragma unroll
      for (int w = 0; w < FW; ++w) tot += red[w];
      const float inv = rsqrtf(tot / (float)a.K + a.eps);
      for (int c = tid; c < K8; c += THREADS) {
        const u32x4 v = x4[c];
        const u32x4 g = w4[c];
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float nlo = rbf(pk_lo(v[e]) * inv), nhi = rbf(pk_hi(v[e]) * inv);
          o[e] = pack2(pk_lo(g[e]) * nlo, pk_hi(g[e]) * nhi);
        }
        xs[XI(c)] = o;
      }
    }
  } else {  // PRO_ATTN: reduce the S split-K partials of every head (flash-decode combine)
    // Every load of a group of 4 splits is issued before the first use: one L2 round trip per group instead of one per
    // split (a runtime-bounded loop of load -> exp -> fma made the prologue S dependent trips long).  The sums run over
    // s = 0, 1, 2, ... in that order, as in k_attn_combine.
    const int S = a.S;
    for (int c = tid; c < K8; c += THREADS) {
      const int head = c >> CSH;     // HC chunks of 8 dims per head (16 at hd 128, 8 at hd 64)
      const int d0 = (c & (HC - 1)) * 8;
      const float* pmh = a.pm + head * S;
      const float* plh = a.pl + head * S;
      float M = -1e30f;
      for (int s0 = 0; s0 < S; s0 += 4) {
        float m4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) m4[j] = (s0 + j < S) ? pmh[s0 + j] : -1e30f;
#pragma unroll
        for (int j = 0; j < 4; ++j) M = fmaxf(M, m4[j]);
      }
      float L = 0.f;
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = 0.f;
      for (int s0 = 0; s0 < S; s0 += 4) {
        float m4[4], l4[4];
        f32x4 p0[4], p1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool ok = s0 + j < S;
          const int sj = ok ? s0 + j : s0;
          m4[j] = ok ? pmh[sj] : -1e30f;
          l4[j] = ok ? plh[sj] : 0.f;
          const f32x4* po4 = reinterpret_cast<const f32x4*>(a.po + ((size_t)(head * S + sj)) * HD + d0);
          p0[j] = po4[0];
          p1[j] = po4[1];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (s0 + j < S) {
            const float w = __expf(m4[j] - M);
            L += w * l4[j];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              o[e] += w * p0[j][e];
              o[4 + e] += w * p1[j][e];
            }
          }
        }
      }
      const float invL = 1.f / L;
      u32x4 ov;
#pragma unroll
      for (int e = 0; e < 4; ++e) ov[e] = pack2(o[2 * e] * invL, o[2 * e + 1] * invL);
      xs[XI(c)] = ov;
    }
  }
  if (F4) {   // the ragged last block's padding: zero codes times zero x (at most 3 pieces; LDS is not zeroed between launches)
    const u32x4 zz = {0u, 0u, 0u, 0u};
    for (int c = K8 + tid; c < 4 * KC; c += THREADS) xs[XI(c)] = zz;
  }
  __syncthreads();

  for (;;) {
    const bool active = unit0 < n_units;  // wave-uniform
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.f;
    // ---- main loop: two register stages (wa holds stage 0 on entry).  W13 under PRO_RMSNORM: one copy of the loop per decode, chosen
    // once per row group (a branch around every stage instead cost the general decode 0.5 us per launch against the loop without it)
#define MAIN_LOOP(NZV) do {                                   \
      constexpr bool NZ = NZV;                                 \
      for (int g = 0; g < G; g += 2) {                         \
        if (g + 1 < G) GLOAD(wb, sb, GIDX(g + 1));             \
        GFMA(wa, sa, GIDX(g));                                 \
        if (g + 1 < G) {                                       \
          if (g + 2 < G) GLOAD(wa, sa, GIDX(g + 2));           \
          GFMA(wb, sb, GIDX(g + 1));                           \
        }                                                      \
      }                                                        \
    } while (0)
    if constexpr (W13 && PRO == PRO_RMSNORM) {
      if (zrow) MAIN_LOOP(false);
      else MAIN_LOOP(true);
    } else {
      MAIN_LOOP(false);
    }
#undef MAIN_LOOP
    const int cur = unit0;
    float q0[R], q1[R];          // this chunk's epilogue operands (the next chunk's are fetched below)
#pragma unroll
    for (int j = 0; j < R; ++j) { q0[j] = pre0[j]; q1[j] = pre1[j]; }
    if (PERSIST) {  // next chunk's first stage goes in flight before this chunk's reduction
      chunk += chunk_stride;
      unit0 = chunk * R;
      if (unit0 < n_units) {
        set_rows(unit0);
        GLOAD(wa, sa, 0);
        if (EPI == EPI_RESID || EPI == EPI_QKV) prefetch_epilogue(unit0);
      }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = wave_sum(acc[r]);
    if (KS > 1) {   // partial sums of the KS waves of a row-chunk meet in LDS; wave ks == 0 adds them in a fixed order
      float* part = red + WAVES;                       // [RW][NR][KS]
      if (lane == 0) {
#pragma unroll
        for (int r = 0; r < NR; ++r) part[(rw * NR + r) * KS + ks] = acc[r];
      }
      __syncthreads();
      if (ks == 0 && lane == 0) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          float t = part[(rw * NR + r) * KS];
#pragma unroll
          for (int k = 1; k < KS; ++k) t += part[(rw * NR + r) * KS + k];
          acc[r] = t;
        }
      }
    }

    // ---- epilogue (one lane per row-chunk; a handful of scalars)
    if (active && lane == 0 && ks == 0) {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const int u = cur + j;
        if (u >= n_units) break;
        gemv_epilogue<EPI, F8, HD>(a, u, PAIRED ? acc[2 * j] : acc[j], PAIRED ? acc[2 * j + 1] : 0.f, q0[j], q1[j], pos);
      }
    }
    if (!PERSIST || unit0 >= n_units) break;
  }
#undef GIDX
#undef GLOAD
#undef GFMA
#undef XI
}

// number of CUs of the current device (cached) — persistent grids are sized from it
static int num_cus() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    hipDeviceProp_t p;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) n = p.multiProcessorCount;
    if (n <= 0) n = 256;
  }
  return n;
}

template <int PRO, int EPI, int R, int U, int WAVES, bool PERSIST, int KS = 1>
static void launch_gemv_t(const GemvArgs& a, hipStream_t s, int blocks_per_cu) {
  int n_units = (EPI == EPI_QKV) ? (a.N >> 1) : (EPI == EPI_SWIGLU ? a.ff : a.N);
  const int per_block = (WAVES / KS) * R;
  int grid = (n_units + per_block - 1) / per_block;
  if (PERSIST) {
    const int cap = num_cus() * (blocks_per_cu > 0 ? blocks_per_cu : 2);
    if (grid > cap) grid = cap;
  }
  const size_t lds = (size_t)(a.K >> 3) * 16 + 64 + 1024;   // x (bf16) + per-wave RMSNorm partials + split-K partials
  if constexpr (EPI == EPI_QKV || PRO == PRO_ATTN) {         // the roles whose layout is per head
    if (a.hd == 64) { hipLaunchKernelGGL((k_gemv<PRO, EPI, R, U, WAVES, PERSIST, false, KS, 64>), dim3(grid), dim3(WAVES * 64), lds, s, a); return; }
  }
  hipLaunchKernelGGL((k_gemv<PRO, EPI, R, U, WAVES, PERSIST, false, KS>), dim3(grid), dim3(WAVES * 64), lds, s, a);
}

// Tuning table: variant -> instantiation.  Variant 0 is the product default for each role; the
// others exist for the in-situ microbenchmark (dtk_bench_gemv) that picked the default.
// The table serves two readers: launch_gemv_variant launches the row, gemv_variant_shape (q != null) only reads its shape - what decides
// a kernel's fold order (U and KS: which k-groups a wave sums; waves: how the RMSNorm prologue folds the sum of squares) - so that
// w13_shape_for below can never disagree with the rows here.
struct GemvShape { int R, U, waves, ks; bool persist; };
#define GV(PRO, EPI, R, U, W, P, BPC) do { if (q) { *q = GemvShape{R, U, W, 1, P}; return; } return launch_gemv_t<PRO, EPI, R, U, W, P>(a, s, BPC); } while (0)
#define GVK(PRO, EPI, R, U, W, KS) do { if (q) { *q = GemvShape{R, U, W, KS, false}; return; } return launch_gemv_t<PRO, EPI, R, U, W, false, KS>(a, s, 0); } while (0)
static void gemv_variant_row(int pro, int epi, int variant, const GemvArgs& a, hipStream_t s, GemvShape* q) {
  if (pro == PRO_RMSNORM && epi == EPI_QKV) {
    switch (variant) {
      default: GV(PRO_RMSNORM, EPI_QKV, 1, 2, 4, false, 0);
      case 8: GV(PRO_RMSNORM, EPI_QKV, 2, 2, 4, false, 0);
      case 9: GV(PRO_RMSNORM, EPI_QKV, 1, 1, 4, false, 0);
      case 10: GV(PRO_RMSNORM, EPI_QKV, 1, 2, 8, false, 0);
      case 11: GV(PRO_RMSNORM, EPI_QKV, 1, 2, 2, false, 0);
      case 1: GV(PRO_RMSNORM, EPI_QKV, 1, 4, 4, false, 0);
      case 2: GV(PRO_RMSNORM, EPI_QKV, 2, 2, 8, false, 0);
      case 3: GV(PRO_RMSNORM, EPI_QKV, 2, 2, 4, true, 4);
      case 4: GV(PRO_RMSNORM, EPI_QKV, 2, 2, 8, true, 2);
      case 5: GV(PRO_RMSNORM, EPI_QKV, 1, 4, 8, true, 2);
      case 6: GV(PRO_RMSNORM, EPI_QKV, 4, 1, 4, false, 0);
      case 7: GV(PRO_RMSNORM, EPI_QKV, 1, 2, 4, false, 0);
    }
  }
  if (pro == PRO_RMSNORM && epi == EPI_SWIGLU) {
    switch (variant) {
      default: GV(PRO_RMSNORM, EPI_SWIGLU, 1, 2, 4, false, 0);
      case 8: GV(PRO_RMSNORM, EPI_SWIGLU, 2, 2, 4, false, 0);
      case 9: GV(PRO_RMSNORM, EPI_SWIGLU, 1, 1, 4, false, 0);
      case 10: GV(PRO_RMSNORM, EPI_SWIGLU, 1, 2, 8, false, 0);
      case 11: GV(PRO_RMSNORM, EPI_SWIGLU, 1, 2, 2, false, 0);
      case 1: GV(PRO_RMSNORM, EPI_SWIGLU, 1, 4, 4, false, 0);
      case 2: GV(PRO_RMSNORM, EPI_SWIGLU, 2, 2, 8, false, 0);
      case 3: GV(PRO_RMSNORM, EPI_SWIGLU, 2, 2, 4, true, 4);
      case 4: GV(PRO_RMSNORM, EPI_SWIGLU, 2, 2, 8, true, 2);
      case 5: GV(PRO_RMSNORM, EPI_SWIGLU, 1, 4, 8, true, 2);
      case 6: GV(PRO_RMSNORM, EPI_SWIGLU, 4, 1, 4, false, 0);
      case 7: GV(PRO_RMSNORM, EPI_SWIGLU, 1, 2, 4, false, 0);
    }
  }
  if (pro == PRO_COPY && epi == EPI_RESID) {
    switch (variant) {
      default: GV(PRO_COPY, EPI_RESID, 1, 8, 4, false, 0);
      case 8: GV(PRO_COPY, EPI_RESID, 2, 4, 4, false, 0);
      case 9: GV(PRO_COPY, EPI_RESID, 1, 2, 4, false, 0);
      case 10: GV(PRO_COPY, EPI_RESID, 1, 8, 8, false, 0);
      case 11: GV(PRO_COPY, EPI_RESID, 1, 8, 2, false, 0);
      case 12: GV(PRO_COPY, EPI_RESID, 1, 4, 2, false, 0);
      case 1: GV(PRO_COPY, EPI_RESID, 1, 4, 4, false, 0);
      case 2: GV(PRO_COPY, EPI_RESID, 4, 2, 4, false, 0);
      case 3: GV(PRO_COPY, EPI_RESID, 2, 4, 8, false, 0);
      case 4: GV(PRO_COPY, EPI_RESID, 2, 4, 4, true, 4);
      case 5: GV(PRO_COPY, EPI_RESID, 2, 4, 8, true, 2);
      case 6: GV(PRO_COPY, EPI_RESID, 1, 8, 4, false, 0);
      case 7: GV(PRO_COPY, EPI_RESID, 2, 2, 4, false, 0);
      // split-K over the waves of a block (KS waves share a row): twice / four times the loads in flight per row
      case 13: GVK(PRO_COPY, EPI_RESID, 1, 4, 8, 2);    // o_proj (K 4096): one k-group per wave, 4 rows per block
      case 14: GVK(PRO_COPY, EPI_RESID, 2, 4, 8, 2);    //                  8 rows per block
      case 15: GVK(PRO_COPY, EPI_RESID, 1, 6, 8, 2);    // down (K 11008): 22 k-iterations = 4 groups of 6, two per wave
      case 16: GVK(PRO_COPY, EPI_RESID, 2, 6, 8, 2);
      case 17: GVK(PRO_COPY, EPI_RESID, 1, 6, 16, 4);   // one group of 6 iterations per wave, 4 rows per 16-wave block
      case 18: GVK(PRO_COPY, EPI_RESID, 1, 2, 16, 4);   // o_proj: 2 iterations per wave
      case 19: GVK(PRO_COPY, EPI_RESID, 1, 3, 8, 2);    // down, 8 groups of 3 iterations
      case 20: GVK(PRO_COPY, EPI_RESID, 1, 4, 4, 2);    // 2 rows per 4-wave block
      case 21: GVK(PRO_COPY, EPI_RESID, 1, 6, 4, 2);
      case 22: GVK(PRO_COPY, EPI_RESID, 4, 2, 8, 2);
    }
  }
  if (pro == PRO_ATTN && epi == EPI_RESID) {   // o_proj that reduces the attention partials in its prologue: fewer, fatter blocks
    switch (variant) {                          // (every block reads ALL partials: H * S * 130 floats)
      default: GV(PRO_ATTN, EPI_RESID, 2, 4, 8, false, 0);   // 16 rows per block
      case 1: GV(PRO_ATTN, EPI_RESID, 2, 4, 4, false, 0);    // 8 rows (the round-1 shape)
      case 2: GV(PRO_ATTN, EPI_RESID, 1, 8, 8, false, 0);    // 8 rows, one per wave
      case 3: GV(PRO_ATTN, EPI_RESID, 4, 2, 8, false, 0);    // 32 rows
      case 4: GV(PRO_ATTN, EPI_RESID, 4, 2, 4, false, 0);    // 16 rows, 4 waves
      case 5: GVK(PRO_ATTN, EPI_RESID, 2, 4, 8, 2);          // 8 rows, split-K 2
      case 6: GVK(PRO_ATTN, EPI_RESID, 4, 4, 8, 2);          // 16 rows, split-K 2
      case 7: GV(PRO_ATTN, EPI_RESID, 2, 4, 16, false, 0);   // 32 rows, 16 waves
      case 8: GVK(PRO_ATTN, EPI_RESID, 2, 4, 16, 2);         // 16 rows, 16 waves, split-K 2
    }
  }
  if (pro == PRO_RMSNORM && epi == EPI_LOGITS) {
    switch (variant) {
      default: GV(PRO_RMSNORM, EPI_LOGITS, 2, 4, 4, false, 0);
      case 1: GV(PRO_RMSNORM, EPI_LOGITS, 4, 2, 8, true, 2);
      case 2: GV(PRO_RMSNORM, EPI_LOGITS, 4, 2, 4, false, 0);
      case 3: GV(PRO_RMSNORM, EPI_LOGITS, 1, 4, 4, false, 0);
      case 4: GV(PRO_RMSNORM, EPI_LOGITS, 1, 8, 4, false, 0);
    }
  }
  if (pro == PRO_RMSNORM && epi == EPI_STORE) {
    if (variant == 20) GV(PRO_RMSNORM, EPI_STORE, 1, 2, 4, false, 0);   // probe: the streaming core + norm prologue only
    GV(PRO_RMSNORM, EPI_STORE, 4, 2, 4, false, 0);
  }
  if (variant == 20) GV(PRO_COPY, EPI_STORE, 1, 2, 4, false, 0);         // probes (dtk_bench_gemv | 0x200): streaming core,
  if (variant == 21) GV(PRO_COPY, EPI_STORE, 1, 8, 4, false, 0);         // plain x copy, plain store
  GV(PRO_COPY, EPI_STORE, 4, 2, 4, false, 0);
}
#undef GV
#undef GVK
void launch_gemv_variant(int pro, int epi, int variant, const GemvArgs& a, hipStream_t s) { gemv_variant_row(pro, epi, variant, a, s, nullptr); }
static GemvShape gemv_variant_shape(int pro, int epi, int variant) {
  GemvShape q{};
  gemv_variant_row(pro, epi, variant, GemvArgs{}, nullptr, &q);
  return q;
}

template <int PRO, int EPI, int R, int U, int WAVES, bool PERSIST = false, int BPC = 4>
static void launch_gemv_f8_t(const GemvArgs& a, hipStream_t s) {
  int n_units = (EPI == EPI_QKV) ? (a.N >> 1) : (EPI == EPI_SWIGLU ? a.ff : a.N);
  const int per_block = WAVES * R;
  int grid = (n_units + per_block - 1) / per_block;
  if (PERSIST && grid > num_cus() * BPC) grid = num_cus() * BPC;
  const size_t lds = (size_t)(a.K >> 3) * 16 + 64 + 1024;
  if constexpr (EPI == EPI_QKV || PRO == PRO_ATTN) {
    if (a.hd == 64) { hipLaunchKernelGGL((k_gemv<PRO, EPI, R, U, WAVES, PERSIST, true, 1, 64>), dim3(grid), dim3(WAVES * 64), lds, s, a); return; }
  }
  hipLaunchKernelGGL((k_gemv<PRO, EPI, R, U, WAVES, PERSIST, true>), dim3(grid), dim3(WAVES * 64), lds, s, a);
}
// fp8-weight decode GEMVs (requires K % 16 == 0); same roles as the bf16 defaults.  An fp8 row is half
// the bytes, so more rows per wave (R=2) amortise the prologue / reduction; DTK_F8_VARIANT sweeps the choice.
static int f8_variant() {
  static int v = -1;
  if (v < 0) { const char* e = getenv("DTK_F8_VARIANT"); v = e ? atoi(e) : 8; }
  return v;
}
#define F8(PRO, EPI, R, U, W) return launch_gemv_f8_t<PRO, EPI, R, U, W>(a, s)
#define F8P(PRO, EPI, R, U, W, BPC) return launch_gemv_f8_t<PRO, EPI, R, U, W, true, BPC>(a, s)
void launch_gemv_f8(int pro, int epi, const GemvArgs& a, hipStream_t s) { launch_gemv_f8_variant(pro, epi, f8_variant(), a, s); }
// the same table with the shape given by the caller (dtk_op_gemv_role: one process reaches every shape)
void launch_gemv_f8_variant(int pro, int epi, int v, const GemvArgs& a, hipStream_t s) {
  if (pro == PRO_RMSNORM && (epi == EPI_QKV || epi == EPI_SWIGLU)) {
    if (epi == EPI_QKV) {
      switch (v) { default: F8(PRO_RMSNORM, EPI_QKV, 2, 2, 4); case 0: F8(PRO_RMSNORM, EPI_QKV, 1, 2, 4);
                   case 2: F8(PRO_RMSNORM, EPI_QKV, 2, 4, 4); case 3: F8(PRO_RMSNORM, EPI_QKV, 4, 2, 4);
                   case 4: F8(PRO_RMSNORM, EPI_QKV, 2, 2, 8); case 5: F8(PRO_RMSNORM, EPI_QKV, 1, 4, 4);
                   case 6: F8P(PRO_RMSNORM, EPI_QKV, 1, 2, 4, 4); case 7: F8P(PRO_RMSNORM, EPI_QKV, 2, 2, 4, 4);
                   case 8: F8P(PRO_RMSNORM, EPI_QKV, 1, 2, 8, 2); case 9: F8P(PRO_RMSNORM, EPI_QKV, 1, 4, 4, 4); }
    }
    switch (v) { default: F8(PRO_RMSNORM, EPI_SWIGLU, 2, 2, 4); case 0: F8(PRO_RMSNORM, EPI_SWIGLU, 1, 2, 4);
                 case 2: F8(PRO_RMSNORM, EPI_SWIGLU, 2, 4, 4); case 3: F8(PRO_RMSNORM, EPI_SWIGLU, 4, 2, 4);
                 case 4: F8(PRO_RMSNORM, EPI_SWIGLU, 2, 2, 8); case 5: F8(PRO_RMSNORM, EPI_SWIGLU, 1, 4, 4);
                 case 6: F8P(PRO_RMSNORM, EPI_SWIGLU, 1, 2, 4, 4); case 7: F8P(PRO_RMSNORM, EPI_SWIGLU, 2, 2, 4, 4);
                 case 8: F8P(PRO_RMSNORM, EPI_SWIGLU, 1, 2, 8, 2); case 9: F8P(PRO_RMSNORM, EPI_SWIGLU, 1, 4, 4, 4); }
  }
  if (pro == PRO_RMSNORM && epi == EPI_LOGITS) {
    switch (v) { default: F8(PRO_RMSNORM, EPI_LOGITS, 4, 2, 4); case 0: F8(PRO_RMSNORM, EPI_LOGITS, 2, 2, 4);
                 case 2: F8(PRO_RMSNORM, EPI_LOGITS, 4, 4, 4); case 3: F8(PRO_RMSNORM, EPI_LOGITS, 8, 2, 4); }
  }
  if (pro == PRO_ATTN && epi == EPI_RESID) F8(PRO_ATTN, EPI_RESID, 2, 2, 4);
  switch (v) { default: F8(PRO_COPY, EPI_RESID, 2, 4, 4); case 0: F8(PRO_COPY, EPI_RESID, 1, 4, 4);
               case 2: F8(PRO_COPY, EPI_RESID, 2, 8, 4); case 3: F8(PRO_COPY, EPI_RESID, 4, 4, 4);
               case 4: F8(PRO_COPY, EPI_RESID, 2, 4, 8); case 5: F8(PRO_COPY, EPI_RESID, 1, 8, 4);
               case 6: F8P(PRO_COPY, EPI_RESID, 1, 4, 4, 4); case 7: F8P(PRO_COPY, EPI_RESID, 2, 4, 4, 4);
               case 8: F8P(PRO_COPY, EPI_RESID, 1, 4, 8, 2); case 9: F8P(PRO_COPY, EPI_RESID, 1, 8, 4, 4); }
}
#undef F8
#undef F8P

// MXFP4-weight decode GEMVs (gemv_inl.h: dot32_f4): the four (prologue, epilogue) pairs of a layer at B = 1 plus the EPI_STORE pair
// of dtk_op_gemv_q4; lm_head stays fp8.  A row is a quarter of its bf16 bytes (K = 4096: 2 KiB = two wave-loads), so the fixed cost
// of a block — the prologue's x, the reduction — weighs more than for fp8.  Shapes by measurement (ds-7b, back-to-back chains over
// all layers, us per launch; DESIGN 3.1c', profiles/mxfp4_shape_sweep_ds-7b.json): the RMSNorm roles run persistent grids sized to the
// machine, R 1, U 2, 8 waves, 2 blocks per CU (gate/up 14.4 against 17.6 for one chunk per wave at R 2, 4 waves; 18.5 / 20.2 for the
// persistent R 2 shapes; q/k/v 11.0 / 10.7 / 14.3 / 12.9); the N = d roles one chunk per wave, R 2, U 2, 4 waves (o_proj 5.4, down 10.0
// against 7.9 / 12.6 for persistent R 1, U 4, 8 waves and 6.8 / 10.7, 6.8 / 13.5 for the other two).  The losing shapes are not built.
template <int PRO, int EPI, int R, int U, int WAVES, bool PERSIST = false, int BPC = 2>
static void launch_gemv_q4_t(const GemvArgs& a, hipStream_t s) {
  int n_units = (EPI == EPI_QKV) ? (a.N >> 1) : (EPI == EPI_SWIGLU ? a.ff : a.N);
  const int per_block = WAVES * R;
  int grid = (n_units + per_block - 1) / per_block;
  if (PERSIST && grid > num_cus() * BPC) grid = num_cus() * BPC;
  const int KC = (a.K + 31) >> 5;
  const size_t lds = (size_t)((4 * KC + 63) & ~63) * 16 + 64 + 1024;   // swizzled x in whole 1 KiB tiles + the RMSNorm partials
  if constexpr (EPI == EPI_QKV || PRO == PRO_ATTN) {
    if (a.hd == 64) { hipLaunchKernelGGL((k_gemv<PRO, EPI, R, U, WAVES, PERSIST, false, 1, 64, true>), dim3(grid), dim3(WAVES * 64), lds, s, a); return; }
  }
  hipLaunchKernelGGL((k_gemv<PRO, EPI, R, U, WAVES, PERSIST, false, 1, 128, true>), dim3(grid), dim3(WAVES * 64), lds, s, a);
}
#define Q4(PRO, EPI, R, U, W) return launch_gemv_q4_t<PRO, EPI, R, U, W>(a, s)
#define Q4P(PRO, EPI, R, U, W, BPC) return launch_gemv_q4_t<PRO, EPI, R, U, W, true, BPC>(a, s)
void launch_gemv_q4(int pro, int epi, const GemvArgs& a, hipStream_t s) {
  if (pro == PRO_RMSNORM && epi == EPI_QKV) Q4P(PRO_RMSNORM, EPI_QKV, 1, 2, 8, 2);
  if (pro == PRO_RMSNORM && epi == EPI_SWIGLU) Q4P(PRO_RMSNORM, EPI_SWIGLU, 1, 2, 8, 2);
  if (pro == PRO_ATTN && epi == EPI_RESID) Q4(PRO_ATTN, EPI_RESID, 2, 2, 4);
  if (pro == PRO_COPY && epi == EPI_RESID) Q4(PRO_COPY, EPI_RESID, 2, 2, 4);
  if (pro == PRO_RMSNORM && epi == EPI_STORE) Q4(PRO_RMSNORM, EPI_STORE, 2, 2, 4);
  if (pro == PRO_COPY && epi == EPI_STORE) Q4(PRO_COPY, EPI_STORE, 2, 2, 4);
  fprintf(stderr, "launch_gemv_q4: no MXFP4 kernel for prologue %d, epilogue %d\n", pro, epi);   // a missing kernel is an error, never a fall-back
  abort();
}
#undef Q4
#undef Q4P

// 13-bit planes of bf16 rows (w13.h; gemv_inl.h: dot8_w13): the four (prologue, epilogue) pairs of a layer, lm_head and the EPI_STORE
// pairs, batch 1.  Variant 0 of a role is what a decode step runs; the others exist for dtk_bench_gemv (| 0x1000), which picked it.
// FW: the waves that fold the RMSNorm sum of squares (k_gemv), 0 = all of the block.
template <int PRO, int EPI, int R, int U, int WAVES, bool PERSIST = false, int KS = 1, int BPC = 2, int FW0 = 0>
static void launch_gemv_w13_t(const GemvArgs& a, hipStream_t s) {
  int n_units = (EPI == EPI_QKV) ? (a.N >> 1) : (EPI == EPI_SWIGLU ? a.ff : a.N);
  const int per_block = (WAVES / KS) * R;
  int grid = (n_units + per_block - 1) / per_block;
  if (PERSIST && grid > num_cus() * BPC) grid = num_cus() * BPC;
  const size_t lds = (size_t)(a.K >> 3) * 16 + 64 + 1024;   // x (bf16, linear) + per-wave RMSNorm partials + split-K partials
  constexpr int FW = FW0 ? FW0 : WAVES;
  if constexpr (EPI == EPI_QKV || PRO == PRO_ATTN) {
    if (a.hd == 64) { hipLaunchKernelGGL((k_gemv<PRO, EPI, R, U, WAVES, PERSIST, false, KS, 64, false, true, FW>), dim3(grid), dim3(WAVES * 64), lds, s, a); return; }
  }
  hipLaunchKernelGGL((k_gemv<PRO, EPI, R, U, WAVES, PERSIST, false, KS, 128, false, true, FW>), dim3(grid), dim3(WAVES * 64), lds, s, a);
}
#define WV(PRO, EPI, R, U, W) return launch_gemv_w13_t<PRO, EPI, R, U, W>(a, s)
#define WVP(PRO, EPI, R, U, W, BPC) return launch_gemv_w13_t<PRO, EPI, R, U, W, true, 1, BPC>(a, s)
#define WVK(PRO, EPI, R, U, W, KS) return launch_gemv_w13_t<PRO, EPI, R, U, W, false, KS>(a, s)
#define WVF(PRO, EPI, R, U, W, BPC, FW) return launch_gemv_w13_t<PRO, EPI, R, U, W, true, 1, BPC, FW>(a, s)   // persistent, norm fold of FW waves
bool gemv_w13_has(int pro, int epi, int v) {
  if (pro == PRO_RMSNORM && (epi == EPI_QKV || epi == EPI_SWIGLU)) return v >= 0 && v <= 7;
  if (pro == PRO_COPY && epi == EPI_RESID) return v >= 0 && v <= 6;
  if (pro == PRO_ATTN && epi == EPI_RESID) return v >= 0 && v <= 2;
  if (pro == PRO_RMSNORM && epi == EPI_LOGITS) return v >= 0 && v <= 7;
  if (pro == PRO_RMSNORM && epi == EPI_STORE) return v >= 0 && v <= 1;
  if (pro == PRO_COPY && epi == EPI_STORE) return v == 0;
  return false;
}
void launch_gemv_w13_variant(int pro, int epi, int v, const GemvArgs& a, hipStream_t s) {
  if (pro == PRO_RMSNORM && epi == EPI_QKV) {
    switch (v) { default: WV(PRO_RMSNORM, EPI_QKV, 1, 4, 4); case 1: WV(PRO_RMSNORM, EPI_QKV, 2, 4, 4); case 2: WV(PRO_RMSNORM, EPI_QKV, 1, 4, 8);
                 case 3: WVP(PRO_RMSNORM, EPI_QKV, 1, 4, 8, 2); case 4: WV(PRO_RMSNORM, EPI_QKV, 1, 8, 4);
                 case 5: WVP(PRO_RMSNORM, EPI_QKV, 1, 4, 4, 4);
                 case 6: WVF(PRO_RMSNORM, EPI_QKV, 1, 4, 8, 2, 4); case 7: WVF(PRO_RMSNORM, EPI_QKV, 1, 4, 16, 1, 4); }   // the 4-wave norm fold in 8 / 16 waves
  }
  if (pro == PRO_RMSNORM && epi == EPI_SWIGLU) {
    switch (v) { default: WV(PRO_RMSNORM, EPI_SWIGLU, 1, 4, 4); case 1: WV(PRO_RMSNORM, EPI_SWIGLU, 2, 4, 4); case 2: WV(PRO_RMSNORM, EPI_SWIGLU, 1, 4, 8);
                 case 3: WVP(PRO_RMSNORM, EPI_SWIGLU, 1, 4, 8, 2); case 4: WV(PRO_RMSNORM, EPI_SWIGLU, 1, 8, 4);
                 case 5: WVP(PRO_RMSNORM, EPI_SWIGLU, 1, 4, 4, 4);
                 case 6: WVF(PRO_RMSNORM, EPI_SWIGLU, 1, 4, 8, 2, 4); case 7: WVF(PRO_RMSNORM, EPI_SWIGLU, 1, 4, 16, 1, 4); }
  }
  if (pro == PRO_COPY && epi == EPI_RESID) {
    switch (v) { default: WV(PRO_COPY, EPI_RESID, 1, 8, 8); case 1: WV(PRO_COPY, EPI_RESID, 1, 4, 8); case 2: WV(PRO_COPY, EPI_RESID, 2, 4, 4);
                 case 3: WVK(PRO_COPY, EPI_RESID, 1, 4, 8, 2); case 4: WVK(PRO_COPY, EPI_RESID, 2, 4, 8, 2);
                 case 5: WV(PRO_COPY, EPI_RESID, 1, 4, 4); case 6: WV(PRO_COPY, EPI_RESID, 1, 4, 16); }
  }
  if (pro == PRO_ATTN && epi == EPI_RESID) {
    switch (v) { default: WVK(PRO_ATTN, EPI_RESID, 2, 4, 16, 2); case 1: WV(PRO_ATTN, EPI_RESID, 2, 4, 8); case 2: WV(PRO_ATTN, EPI_RESID, 2, 4, 4); }
  }
  if (pro == PRO_RMSNORM && epi == EPI_LOGITS) {
    switch (v) { default: WV(PRO_RMSNORM, EPI_LOGITS, 1, 4, 4); case 1: WV(PRO_RMSNORM, EPI_LOGITS, 2, 4, 4); case 2: WVP(PRO_RMSNORM, EPI_LOGITS, 1, 4, 8, 2);
                 case 3: WVP(PRO_RMSNORM, EPI_LOGITS, 2, 4, 8, 2); case 4: WV(PRO_RMSNORM, EPI_LOGITS, 2, 4, 8);
                 case 5: WVF(PRO_RMSNORM, EPI_LOGITS, 2, 4, 8, 2, 4); case 6: WVF(PRO_RMSNORM, EPI_LOGITS, 1, 4, 8, 2, 4);
                 case 7: WVF(PRO_RMSNORM, EPI_LOGITS, 2, 4, 16, 1, 4); }
  }
  if (pro == PRO_RMSNORM && epi == EPI_STORE) { if (v == 1) WVF(PRO_RMSNORM, EPI_STORE, 2, 4, 8, 2, 4); WV(PRO_RMSNORM, EPI_STORE, 2, 4, 4); }
  if (pro == PRO_COPY && epi == EPI_STORE) WV(PRO_COPY, EPI_STORE, 2, 4, 4);
  fprintf(stderr, "launch_gemv_w13: no 13-bit kernel for prologue %d, epilogue %d\n", pro, epi);   // a missing kernel is an error, never a fall-back
  abort();
}
#undef WV
#undef WVP
#undef WVK
#undef WVF
// The 13-bit shape launch_gemv streams a.Wp in when the role's bf16 variant is `v`, or -1 = the bf16 rows stay.  The shape must give the
// bf16 variant's bits, and two things of a shape enter them.  (1) The fold of a row: without split-K it is gemv_inl.h's whatever the
// shape; a split-K variant deals k-groups of U iterations to KS waves, and only U = 4, KS = 2 has a 13-bit twin (a stage is whole sign
// blocks: U % 4 == 0), so any other split-K choice keeps bf16.  (2) PRO_RMSNORM: the sum of squares is folded per thread, per wave and
// over the waves, so it depends on how many waves fold - the 13-bit shape folds with the bf16 variant's number of waves, which is its
// own block's or, in the shapes built with k_gemv's FW (q/k/v, gate/up 6 and 7, lm_head 5 to 7, STORE 1), that of a 4-wave block in a
// persistent block of 8 or 16 (a 16-wave shape folding with all 16 changed `inv` in the last place at K = 4096 and with it a token of the
// benchmark's rollout).
// Defaults by measurement among those (ds-7b, back-to-back chains over all layers' weights, us per launch, bf16 kernel -> 13-bit shape;
// DESIGN 3.1c'', profiles/w13_ds-7b.json): q/k/v 18.20 -> 17.11 and gate/up 28.41 -> 26.14 (persistent, R 1, U 4, 4 waves, 4 blocks per
// CU; one chunk per wave 19.3 / 27.2, R 2 18.6 / 32.9, U 8 = one stage 22.9 / 30.5); down 17.66 -> 15.46 (R 1, U 4, 8 waves; 16.10 at U 8,
// 15.81 with 4 waves, 18.2 split-K); lm_head 37.73 -> 36.40 (R 2, U 4, 4 waves; 37.9 at R 1).  With the short decode of rows without a zero
// code and the 4-wave fold in larger blocks (one later visit, same chains): q/k/v 17.37 -> 16.82 in the same shape and 16.37 persistent
// in 8 waves (shape 6; 16.61 in 16), gate/up 27.14 -> 25.72 in the same shape (26.15 / 26.58 in shapes 6 / 7), lm_head 36.25 -> 34.64 in
// the same shape and 33.53 persistent in 8 waves, R 2 (shape 5; 34.70 at R 1, 34.60 in 16 waves).  o_proj (33.6 MB, latency-bound) is SLOWER on planes in every shape tried
// (7.76 -> 8.03 at best): it keeps its bf16 rows.
static int w13_shape_for(int pro, int epi, int v, const GemvArgs& a) {
  const GemvShape sh = gemv_variant_shape(pro, epi, v);              // the bf16 row's own shape, from the table that launches it
  if (pro == PRO_ATTN) return -1;                                    // o_proj
  if (pro == PRO_COPY && epi == EPI_RESID) {
    if (a.K == a.d) return -1;                                       // o_proj behind the combine kernel
    if (sh.ks == 1) return 1;
    return (sh.ks == 2 && sh.U == 4) ? 3 : -1;                       // split-K 2 over groups of 4 iterations has a twin; nothing else
  }
  // K >= 4096 (where the chains were run): q/k/v and lm_head in the persistent 8-wave shapes that fold the norm as the 4-wave bf16 kernel does
  const bool big = a.K >= 4096;
  if (pro == PRO_RMSNORM && epi == EPI_QKV) return sh.waves == 4 ? (big ? 6 : 5) : (sh.waves == 8 ? 3 : -1);
  if (pro == PRO_RMSNORM && epi == EPI_SWIGLU) return sh.waves == 4 ? 5 : (sh.waves == 8 ? 3 : -1);
  if (pro == PRO_RMSNORM && epi == EPI_LOGITS) return sh.waves == 4 ? (big ? 5 : 1) : (sh.waves == 8 ? 4 : -1);
  if (pro == PRO_RMSNORM && epi == EPI_STORE) return sh.waves == 4 ? 0 : -1;
  if (pro == PRO_COPY && epi == EPI_STORE) return 0;
  return -1;
}

// Packs [N][K] bf16 rows into 13-bit planes (w13.h), a block per row: hb = the row's largest e >> 1, then a thread per (sign block,
// lane) writes its four chunks' pieces of the three planes.  A row with a weight below the window adds 1 to *bad_rows (the caller then
// drops the matrix' packed copy; such weights are written as zero, never as another value).  W is only read.  The row byte Wh is
// w13.h's device byte: hb, and W13_ZROW if a weight of the row has e >> 1 == 0 (`zflag_all`: in every row - the kernels then decode
// every row by the general rule; option "w13_nz" = 0).
__global__ __launch_bounds__(256) void k_pack_w13_rows(const bf16_t* W, uint8_t* Wp, uint8_t* Wh, unsigned* bad_rows, int N, int K, int zflag_all) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const u32x4* w4 = reinterpret_cast<const u32x4*>(W + (size_t)row * K);
  unsigned char* out = Wp + (size_t)row * w13_row_bytes(K);
  __shared__ int red[4], redq[4];
  __shared__ int any_bad;
  const int K8 = K >> 3, J2 = w13_units(K), J4 = w13_blocks(K);
  int hb = 0, qmin = 127;                      // the row's largest and smallest e >> 1
  for (int c = tid; c < K8; c += 256) {
    const u32x4 v = w4[c];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q0 = (int)((v[e] >> 8) & 0x7fu), q1 = (int)((v[e] >> 24) & 0x7fu);
      hb = max(hb, max(q0, q1));
      qmin = min(qmin, min(q0, q1));
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { hb = max(hb, __shfl_xor(hb, off)); qmin = min(qmin, __shfl_xor(qmin, off)); }
  if ((tid & 63) == 0) { red[tid >> 6] = hb; redq[tid >> 6] = qmin; }
  if (tid == 0) any_bad = 0;
  __syncthreads();
  hb = max(max(red[0], red[1]), max(red[2], red[3]));
  qmin = min(min(redq[0], redq[1]), min(redq[2], redq[3]));
  if (tid == 0) Wh[row] = (uint8_t)(hb | ((qmin == 0 || zflag_all) ? W13_ZROW : 0));
  const int lo = w13_lo(hb);
  int bad = 0;
  for (int t = tid; t < J4 * 64; t += 256) {
    const int b = t >> 6, l = t & 63;
    uint32_t sg = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = 2 * b + h;
      if (j >= J2) break;
      u32x4 lv;
      u32x2 nv;
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2) {
        const int i = 2 * h + i2, c = 256 * b + 64 * i + l;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (c < K8) v = w4[c];
        uint32_t la = 0, lb = 0, n = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          unsigned wk = (v[k >> 1] >> (16 * (k & 1))) & 0xffffu;
          int code = w13_code(wk, lo);
          if (code < 0) { ++bad; code = 0; wk = 0; }
          const int kb = 8 * (k & 3);
          if (k < 4) la |= (wk & 0xffu) << kb; else lb |= (wk & 0xffu) << kb;
          n |= (uint32_t)code << (kb + 4 * (k >> 2));
          sg |= (wk >> 15) << (kb + 2 * i + (k >> 2));
        }
        lv[2 * i2] = la; lv[2 * i2 + 1] = lb; nv[i2] = n;
      }
      reinterpret_cast<u32x4*>(out)[j * 64 + l] = lv;
      reinterpret_cast<u32x2*>(out + w13_n_off(K))[j * 64 + l] = nv;
    }
    reinterpret_cast<uint32_t*>(out + w13_s_off(K))[b * 64 + l] = sg;
  }
  if (bad) atomicOr(&any_bad, 1);
  __syncthreads();
  if (tid == 0 && any_bad) atomicAdd(bad_rows, 1u);
}
void launch_pack_w13_rows(const bf16_t* W, uint8_t* Wp, uint8_t* Wh, unsigned* bad_rows, int N, int K, bool zflag_all, hipStream_t s) {
  hipLaunchKernelGGL(k_pack_w13_rows, dim3(N), dim3(256), 0, s, W, Wp, Wh, bad_rows, N, K, zflag_all ? 1 : 0);
}

// per-role default variant (tuned): indexed by epilogue; slot 5 = o_proj (EPI_RESID with K == d) when it has its own choice
// (-1: same as EPI_RESID), slot 6 = o_proj with the PRO_ATTN prologue
static int g_variant[8] = {0, 0, 0, 0, 0, -1, 0, 0};
void set_gemv_default_variant(int epi, int variant) { if (epi >= 0 && epi < 8) g_variant[epi] = variant; }

// the bf16 variant of a role at this shape: the caller's (dtk_set_gemv_variant) or the measured default
static int gemv_chosen_variant(int pro, int epi, const GemvArgs& a) {
  // PRO_ATTN, 0 = not chosen: 16 rows per 16-wave block with split-K 2 (d > 2048: 387.0 tok/s vs 385.9), 8 rows per block (d <= 2048)
  if (pro == PRO_ATTN) return g_variant[6] ? g_variant[6] : (a.d > 2048 ? 8 : 1);
  int v = g_variant[epi & 7];
  const bool o_proj = epi == EPI_RESID && a.K == a.d;
  if (o_proj && g_variant[5] >= 0) v = g_variant[5];
  // Measured defaults (tools/tune_decode.py, profiles/r02_tune_decode_*.log); variant 0 of a role = "not chosen by the caller".
  if (v == 0 && a.d > 0 && a.d <= 2048) {
    // d <= 2048 (ds-1.3b): every kernel streams 8-45 MB and sits on its ~4 us launch + latency floor
    if (epi == EPI_SWIGLU) v = 5;                    // (R 1, U 4, 8 waves, persistent, 2 blocks per CU): 9.8 us vs 10.3
    else if (epi == EPI_RESID) v = o_proj ? 1 : 15;  // o_proj (R 1, U 4, 4 waves) 4.08 us; down split-K 2 (R 1, U 6, 8 waves) 6.88 vs 7.41
    else if (epi == EPI_LOGITS) v = 3;               // (R 1, U 4, 4 waves) 20.0 us vs 21.9
  } else if (v == 0 && a.d > 2048) {
    if (epi == EPI_RESID) v = 10;                    // (R 1, U 8, 8 waves): o_proj 7.76 us, down 17.67; whole step 380 -> 383 tok/s
    else if (epi == EPI_LOGITS) v = 3;               // 37.9 us vs 38.9
  }
  return v;
}

void launch_gemv(int pro, int epi, const GemvArgs& a, hipStream_t s) {
  if (a.W4) return launch_gemv_q4(pro, epi, a, s);
  if (a.W8) return launch_gemv_f8(pro, epi, a, s);
  const int v = gemv_chosen_variant(pro, epi, a);
  // a.Wp (13-bit planes of a.W): the shape that folds in the order of bf16 variant v, so the sums stay that kernel's bits; where no
  // such shape exists the bf16 rows are streamed (gemv_w13_takes tells the packer, which then keeps no planes)
  const int v13 = a.Wp ? w13_shape_for(pro, epi, v, a) : -1;
  if (v13 >= 0) return launch_gemv_w13_variant(pro, epi, v13, a, s);
  launch_gemv_variant(pro, epi, v, a, s);
}
bool gemv_w13_takes(int pro, int epi, const GemvArgs& a) { return w13_shape_for(pro, epi, gemv_chosen_variant(pro, epi, a), a) >= 0; }

// ------------------------------------------------------------------------------------------
// Decode attention, split-K ("flash-decode"): grid (H, S).  Block (h, s) scans keys
// [s*chunk, (s+1)*chunk) of head h: 16 lanes share one 256-byte K/V row (16 B each), so a
// wave covers 4 rows per load instruction and a block 16 rows; every 16-lane group keeps
// its own online-softmax stream (m, l, o[8 dims]); streams merge through shuffles + LDS.
// Scores and probabilities stay fp32 (fused-attention semantics: one bf16 rounding of the
// head output, done by the consumer's PRO_ATTN prologue).
__global__ __launch_bounds__(256) void k_attn_decode(AttnDecArgs a) {
  const int h = blockIdx.x, sp = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = lane & 15;   // which 16-byte piece of the row
  const int grp = lane >> 4;   // which of the wave's 4 rows
  const int n = a.st->pos + 1; // keys 0..pos (this step's k/v were appended by the QKV kernel)
  int chunk = (n + a.S - 1) / a.S;
  chunk = (chunk + 15) & ~15;
  const int j_begin = sp * chunk;
  const int j_end = min(n, j_begin + chunk);

  // q piece of this lane: dims sub*8 .. sub*8+7 as packed bf16
  const u32x4 qv = reinterpret_cast<const u32x4*>(a.q + h * 128)[sub];
  const int kvh = h / a.G;   // GQA: G query heads share one kv head
  const bf16_t* kbase = a.kcache + (size_t)kvh * a.T_max * 128;
  const bf16_t* vbase = a.vcache + (size_t)kvh * a.T_max * 128;

  float m = -1e30f, l = 0.f;
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;

  // 64 rows per block iteration: every 16-lane group has 4 K rows + 4 V rows (8 x 16 B per lane)
  // in flight before the first dot product, so a ~500-token context is one memory round trip
  for (int j0 = j_begin; j0 < j_end; j0 += 64) {
    u32x4 kv[4], vv[4];
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = j0 + i * 16 + wave * 4 + grp;
      ok[i] = j < j_end;
      const int jj = ok[i] ? j : j_begin;  // clamp: always a valid row
      kv[i] = reinterpret_cast<const u32x4*>(kbase + (size_t)jj * 128)[sub];
      vv[i] = reinterpret_cast<const u32x4*>(vbase + (size_t)jj * 128)[sub];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s = dot8(qv, kv[i], 0.f);
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
      s += __shfl_xor(s, 8, 64);
      s *= a.scale;
      if (ok[i]) {
        const float mn = fmaxf(m, s);
        const float corr = __expf(m - mn);
        const float p = __expf(s - mn);
        l = l * corr + p;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[2 * e] = o[2 * e] * corr + p * pk_lo(vv[i][e]);
          o[2 * e + 1] = o[2 * e + 1] * corr + p * pk_hi(vv[i][e]);
        }
        m = mn;
      }
    }
  }
  // merge the 4 row-groups of the wave (lanes with equal sub)
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    const float m2 = __shfl_xor(m, off, 64);
    const float l2 = __shfl_xor(l, off, 64);
    const float mn = fmaxf(m, m2);
    const float c1 = __expf(m - mn), c2 = __expf(m2 - mn);
    l = l * c1 + l2 * c2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float o2 = __shfl_xor(o[e], off, 64);
      o[e] = o[e] * c1 + o2 * c2;
    }
    m = mn;
  }
  // merge the 4 waves through LDS
  __shared__ float sm_m[4][16], sm_l[4][16], sm_o[4][16][8];
  if (grp == 0) {
    sm_m[wave][sub] = m;
    sm_l[wave][sub] = l;
#pragma unroll
    for (int e = 0; e < 8; ++e) sm_o[wave][sub][e] = o[e];
  }
  __syncthreads();
  if (tid < 16) {
    float M = sm_m[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) M = fmaxf(M, sm_m[w][tid]);
    float L = 0.f;
    float oo[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) oo[e] = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float c = __expf(sm_m[w][tid] - M);
      L += c * sm_l[w][tid];
#pragma unroll
      for (int e = 0; e < 8; ++e) oo[e] += c * sm_o[w][tid][e];
    }
    const size_t slot = (size_t)h * a.S + sp;
    if (a.combine != 1) {  // partials for k_attn_combine / the consumer-side combine (k_gemv<PRO_ATTN>)
      float* dst = a.po + slot * 128 + tid * 8;
#pragma unroll
      for (int e = 0; e < 8; ++e) dst[e] = oo[e];
      if (tid == 0) {
        a.pm[slot] = M;
        a.pl[slot] = L;
      }
      return;
    }
    // ---- in-kernel combine by the last-arriving split of this head (placement independent):
    // partials are published with 8-byte agent-scope (write-through, sc1) stores, drained, then
    // one relaxed agent-scope ticket; the block that draws S-1 reads them back with agent-scope
    // loads (guide: "8-B agent atomics both sides"), normalises, rounds once to bf16.
    typedef unsigned long long u64;
    u64* part = reinterpret_cast<u64*>(a.po) + slot * 65;  // 64 x {o,o} + {m,l}
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const u64 v = (u64)__float_as_uint(oo[2 * e]) | ((u64)__float_as_uint(oo[2 * e + 1]) << 32);
      __hip_atomic_store(part + tid * 4 + e, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid == 0) {
      const u64 v = (u64)__float_as_uint(M) | ((u64)__float_as_uint(L) << 32);
      __hip_atomic_store(part + 64, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing lane is in this wave
    unsigned ticket = 0;
    if (tid == 0) ticket = __hip_atomic_fetch_add(a.counters + h, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ticket = __shfl(ticket, 0, 64);
    if (ticket != (unsigned)(a.S - 1)) return;
    const u64* base = reinterpret_cast<u64*>(a.po) + (size_t)h * a.S * 65;
    float Mg = -1e30f;
    for (int s = 0; s < a.S; ++s) {
      const u64 v = __hip_atomic_load(base + (size_t)s * 65 + 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      Mg = fmaxf(Mg, __uint_as_float((unsigned)v));
    }
    float Lg = 0.f;
    float og[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) og[e] = 0.f;
    for (int s = 0; s < a.S; ++s) {
      const u64 mlv = __hip_atomic_load(base + (size_t)s * 65 + 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const float w = __expf(__uint_as_float((unsigned)mlv) - Mg);
      Lg += w * __uint_as_float((unsigned)(mlv >> 32));
      const u64* src = base + (size_t)s * 65 + tid * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const u64 v = __hip_atomic_load(src + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        og[2 * e] += w * __uint_as_float((unsigned)v);
        og[2 * e + 1] += w * __uint_as_float((unsigned)(v >> 32));
      }
    }
    const float invL = 1.f / Lg;
    u32x4 ov;
#pragma unroll
    for (int e = 0; e < 4; ++e) ov[e] = pack2(og[2 * e] * invL, og[2 * e + 1] * invL);
    reinterpret_cast<u32x4*>(a.out + h * 128)[tid] = ov;
    if (tid == 0) __hip_atomic_store(a.counters + h, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Reduction of the S split-K partials of every head: one HD-thread block per head, thread = dim.
// A kernel boundary (not an in-launch hand-off) publishes the partials: measured cheaper than both
// the consumer-side combine in o_proj's prologue (133 KB re-read by every block) and a
// last-arriver combine inside k_attn_decode (agent-scope stores + ticket + serialized loads).
template <int HD = 128>
__global__ __launch_bounds__(HD) void k_attn_combine(AttnDecArgs a) {
  const int h = blockIdx.x, t = threadIdx.x;
  const int S = a.S;
  // all loads first (one memory round trip), then the arithmetic
  float pm[16], pl[16], po[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const bool ok = s < S;
    const int ss = ok ? s : 0;
    pm[s] = ok ? a.pm[h * S + ss] : -1e30f;
    pl[s] = ok ? a.pl[h * S + ss] : 0.f;
    po[s] = ok ? a.po[((size_t)(h * S + ss)) * HD + t] : 0.f;
  }
  float M = -1e30f;
#pragma unroll
  for (int s = 0; s < 16; ++s) M = fmaxf(M, pm[s]);
  float L = 0.f, o = 0.f;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const float w = __expf(pm[s] - M);
    L += w * pl[s];
    o += w * po[s];
  }
  a.out[h * HD + t] = f2bf(o / L);
}

// Short-context variant: ONE 1024-thread block per head scans all keys (16 waves x 4 row-groups, 4 rows
// each in flight = 256 rows per iteration), merges its 64 online-softmax streams through shuffles + LDS
// and writes the normalised bf16 head output itself: no split-K partials, no combine kernel (2 launches
// and ~4 us per layer less below ~1k tokens of context; above that the split-K grid wins on bandwidth).
__global__ __launch_bounds__(1024) void k_attn_decode_head(AttnDecArgs a) {
  const int h = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = lane & 15, grp = lane >> 4;
  const int n = a.st->pos + 1;
  const u32x4 qv = reinterpret_cast<const u32x4*>(a.q + h * 128)[sub];
  const int kvh = h / a.G;   // GQA: G query heads share one kv head
  const bf16_t* kbase = a.kcache + (size_t)kvh * a.T_max * 128;
  const bf16_t* vbase = a.vcache + (size_t)kvh * a.T_max * 128;
  float m = -1e30f, l = 0.f;
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
  for (int j0 = 0; j0 < n; j0 += 256) {
    u32x4 kv[4], vv[4];
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = j0 + i * 64 + wave * 4 + grp;
      ok[i] = j < n;
      const int jj = ok[i] ? j : 0;
      kv[i] = reinterpret_cast<const u32x4*>(kbase + (size_t)jj * 128)[sub];
      vv[i] = reinterpret_cast<const u32x4*>(vbase + (size_t)jj * 128)[sub];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s = dot8(qv, kv[i], 0.f);
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
      s += __shfl_xor(s, 8, 64);
      s *= a.scale;
      if (ok[i]) {
        const float mn = fmaxf(m, s);
        const float corr = __expf(m - mn);
        const float p = __expf(s - mn);
        l = l * corr + p;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[2 * e] = o[2 * e] * corr + p * pk_lo(vv[i][e]);
          o[2 * e + 1] = o[2 * e + 1] * corr + p * pk_hi(vv[i][e]);
        }
        m = mn;
      }
    }
  }
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    const float m2 = __shfl_xor(m, off, 64);
    const float l2 = __shfl_xor(l, off, 64);
    const float mn = fmaxf(m, m2);
    const float c1 = __expf(m - mn), c2 = __expf(m2 - mn);
    l = l * c1 + l2 * c2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float o2 = __shfl_xor(o[e], off, 64);
      o[e] = o[e] * c1 + o2 * c2;
    }
    m = mn;
  }
  __shared__ float sm_m[16][16], sm_l[16][16], sm_o[16][16][8];
  if (grp == 0) {
    sm_m[wave][sub] = m;
    sm_l[wave][sub] = l;
#pragma unroll
    for (int e = 0; e < 8; ++e) sm_o[wave][sub][e] = o[e];
  }
  __syncthreads();
  if (tid < 16) {
    float M = sm_m[0][tid];
#pragma unroll
    for (int w = 1; w < 16; ++w) M = fmaxf(M, sm_m[w][tid]);
    float L = 0.f;
    float oo[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) oo[e] = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const float c = __expf(sm_m[w][tid] - M);
      L += c * sm_l[w][tid];
#pragma unroll
      for (int e = 0; e < 8; ++e) oo[e] += c * sm_o[w][tid][e];
    }
    const float invL = 1.f / L;
    u32x4 ov;
#pragma unroll
    for (int e = 0; e < 4; ++e) ov[e] = pack2(oo[2 * e] * invL, oo[2 * e + 1] * invL);
    reinterpret_cast<u32x4*>(a.out + h * 128)[tid] = ov;
  }
}

// Position-independent split scheme (variant 1): the keys are cut into tiles of ROWS = 16 * WAVES rows and tile t belongs to
// split t % S, so a block knows its first tile WITHOUT the position: its K/V loads (and q) go in flight before `pos` has
// been read — one dependent memory trip less on the critical path of a latency-bound kernel — and are masked once it has.
// THREADS = 256 / 512 / 1024 trades blocks for rows per memory round trip (64 / 128 / 256); with S splits one round trip
// covers S * ROWS keys.  S == 1 writes the normalised bf16 head output itself (no partials, no combine).
// HD = 128: a K / V row is 256 B = 16 lanes x 16 B, a wave-load covers 4 rows.  HD = 64 (TinyLlama): a row is 128 B = 8 lanes x
// 16 B, a wave-load covers 8 rows and each of the 8 lane groups keeps its own online-softmax stream (ROWS = 32 * WAVES).
template <int THREADS, int HD = 128>
__global__ __launch_bounds__(THREADS) void k_attn_decode_t(AttnDecArgs a) {
  static_assert(HD == 128 || HD == 64, "head dim 128 or 64");
  constexpr int LPR = HD / 8;                  // lanes per K / V row (16 B each)
  constexpr int GPW = 64 / LPR;                // row groups per wave (rows per wave-load)
  constexpr int LSH = HD == 128 ? 4 : 3;       // log2(LPR)
  constexpr int WAVES = THREADS / 64, ROWS = WAVES * GPW * 4;
  const int h = blockIdx.x, sp = blockIdx.y, S = a.S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = lane & (LPR - 1), grp = lane >> LSH;
  const int kvh = h / a.G;
  const bf16_t* kbase = a.kcache + (size_t)kvh * a.T_max * HD;
  const bf16_t* vbase = a.vcache + (size_t)kvh * a.T_max * HD;
  u32x4 kv[4], vv[4];
  auto load_tile = [&](int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int j = t * ROWS + i * (ROWS / 4) + wave * GPW + grp;
      j = min(j, a.T_max - 1);        // always a row of the cache; rows at or beyond the context are masked below
      kv[i] = ld_nt(reinterpret_cast<const u32x4*>(kbase + (size_t)j * HD) + sub);      // a K / V row is read once per token by one block:
      vv[i] = ld_nt(reinterpret_cast<const u32x4*>(vbase + (size_t)j * HD) + sub);      // non-temporal, like the weights
    }
  };
  int t = sp;
  load_tile(t);
  const u32x4 qv = reinterpret_cast<const u32x4*>(a.q + h * HD)[sub];
  const int n = a.st->pos + 1;        // keys 0..pos (this step's k/v were appended by the QKV kernel)

  float m = -1e30f, l = 0.f;
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
  while (t * ROWS < n) {
    u32x4 kc[4], vc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { kc[i] = kv[i]; vc[i] = vv[i]; }
    const int tcur = t;
    t += S;
    if (t * ROWS < n) load_tile(t);   // contexts beyond S * ROWS keys: next tile in flight under this one's arithmetic
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = tcur * ROWS + i * (ROWS / 4) + wave * GPW + grp;
      float s = dot8(qv, kc[i], 0.f);
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
      if (LPR == 16) s += __shfl_xor(s, 8, 64);
      s *= a.scale;
      if (j < n) {
        const float mn = fmaxf(m, s);
        const float corr = __expf(m - mn);
        const float p = __expf(s - mn);
        l = l * corr + p;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[2 * e] = o[2 * e] * corr + p * pk_lo(vc[i][e]);
          o[2 * e + 1] = o[2 * e + 1] * corr + p * pk_hi(vc[i][e]);
        }
        m = mn;
      }
    }
  }
  // merge the GPW row-groups of the wave (lanes with equal sub)
#pragma unroll
  for (int off = LPR; off <= 32; off <<= 1) {
    const float m2 = __shfl_xor(m, off, 64);
    const float l2 = __shfl_xor(l, off, 64);
    const float mn = fmaxf(m, m2);
    const float c1 = __expf(m - mn), c2 = __expf(m2 - mn);
    l = l * c1 + l2 * c2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float o2 = __shfl_xor(o[e], off, 64);
      o[e] = o[e] * c1 + o2 * c2;
    }
    m = mn;
  }
  __shared__ float sm_m[WAVES][LPR], sm_l[WAVES][LPR], sm_o[WAVES][LPR][8];
  if (grp == 0) {
    sm_m[wave][sub] = m;
    sm_l[wave][sub] = l;
#pragma unroll
    for (int e = 0; e < 8; ++e) sm_o[wave][sub][e] = o[e];
  }
  __syncthreads();
  if (tid < LPR) {
    float M = sm_m[0][tid];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) M = fmaxf(M, sm_m[w][tid]);
    float L = 0.f;
    float oo[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) oo[e] = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const float c = __expf(sm_m[w][tid] - M);
      L += c * sm_l[w][tid];
#pragma unroll
      for (int e = 0; e < 8; ++e) oo[e] += c * sm_o[w][tid][e];
    }
    if (S == 1) {     // the whole head in this block: normalise and round once, no partials
      const float invL = 1.f / L;
      u32x4 ov;
#pragma unroll
      for (int e = 0; e < 4; ++e) ov[e] = pack2(oo[2 * e] * invL, oo[2 * e + 1] * invL);
      reinterpret_cast<u32x4*>(a.out + h * HD)[tid] = ov;
      return;
    }
    const size_t slot = (size_t)h * S + sp;   // partials for k_attn_combine / the consumer-side combine (k_gemv<PRO_ATTN>)
    f32x4* dst = reinterpret_cast<f32x4*>(a.po + slot * HD + tid * 8);
    dst[0] = (f32x4){oo[0], oo[1], oo[2], oo[3]};
    dst[1] = (f32x4){oo[4], oo[5], oo[6], oo[7]};
    if (tid == 0) {
      a.pm[slot] = M;         // a split without a key below the context keeps M = -1e30, L = 0: weight exp(-1e30 - max) = 0
      a.pl[slot] = L;
    }
  }
}

void launch_attn_decode(const AttnDecArgs& a, hipStream_t s) {
  if (a.hd == 64) {  // TinyLlama: the tile kernel and the combine kernel only (dtk_set_option refuses attn_threads 0 at hd 64)
    if (!a.threads) return;
    const dim3 grid(a.H, a.S);
    if (a.threads >= 1024) hipLaunchKernelGGL((k_attn_decode_t<1024, 64>), grid, dim3(1024), 0, s, a);
    else if (a.threads >= 512) hipLaunchKernelGGL((k_attn_decode_t<512, 64>), grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL((k_attn_decode_t<256, 64>), grid, dim3(256), 0, s, a);
    if (a.S > 1 && a.combine == 2) hipLaunchKernelGGL(k_attn_combine<64>, dim3(a.H), dim3(64), 0, s, a);
    return;
  }
  if (a.threads) {   // tile-interleaved splits (k_attn_decode_t); a.combine: 0 consumer reduces the partials, 2 own kernel; S == 1: direct
    const dim3 grid(a.H, a.S);
    if (a.threads >= 1024) hipLaunchKernelGGL(k_attn_decode_t<1024>, grid, dim3(1024), 0, s, a);
    else if (a.threads >= 512) hipLaunchKernelGGL(k_attn_decode_t<512>, grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL(k_attn_decode_t<256>, grid, dim3(256), 0, s, a);
    if (a.S > 1 && a.combine == 2) hipLaunchKernelGGL(k_attn_combine<128>, dim3(a.H), dim3(128), 0, s, a);
    return;
  }
  if (a.combine == 3) {  // one block per head, output written directly
    hipLaunchKernelGGL(k_attn_decode_head, dim3(a.H), dim3(1024), 0, s, a);
    return;
  }
  hipLaunchKernelGGL(k_attn_decode, dim3(a.H, a.S), dim3(256), 0, s, a);
  if (a.combine == 2) hipLaunchKernelGGL(k_attn_combine<128>, dim3(a.H), dim3(128), 0, s, a);
}

// ------------------------------------------------------------------------------------------
// Sampler: HF logits processors + argmax | multinomial for ONE sequence, one 1024-thread
// block (the logits are 126-513 KB and L2 resident).  Mirrors generation/utils.py _sample:
// NoBadWords(-inf) -> SuppressTokensAtBegin(-inf on the first generated token) ->
// Temperature -> TopK -> TopP -> softmax -> draw.  Top-k/top-p thresholds come from a
// 4x8-bit radix descent over order-preserving keys with fixed-point (integer) probability
// mass, so the kept set and the inverse-CDF draw are deterministic and reproducible by
// oracle/sampling.py.  The block then advances DecState and gathers the token embedding
// into the residual stream (first op of the next forward).
#define SAMPLE_THREADS 1024

__device__ __forceinline__ bool is_banned(const SamplingDev* sp, int i, bool first) {
  for (int k = 0; k < sp->n_bad; ++k)
    if (sp->bad_ids[k] == i) return true;
  for (int k = 0; k < sp->n_always; ++k)
    if (sp->always_ids[k] == i) return true;
  if (first)
    for (int k = 0; k < sp->n_begin; ++k)
      if (sp->begin_ids[k] == i) return true;
  return false;
}

// LP (SampleArgs::lp_ring, dtk_set_option "logprobs"): the token's (logprob, sample_logprob) next to it.  Pass 1 carries an online
// log-sum-exp of the RAW logits (no mask, no temperature) beside the masked maximum — no further walk over the row; the pair is
// computed and stored by thread 0.  LP = false is the kernel as it was before the option existed.
// TR (SampleArgs::trunc, dtk_set_sampling_ext): min-p and the epsilon cut-off behind top-p, both thresholds on the integer masses.
// min-p keeps q >= SamplingDev::qmin; epsilon keeps q >= (int64)((double)eps * (double)total_m), total_m the mass kept so far (one more
// block reduction).  Both fold into one mass floor; a floor above 2^31 (epsilon left nothing) keeps the first arg-max alone.
// TR = false is the kernel as it was before the two values existed.
// PN (SampleArgs::pen, dtk_set_penalties): the logit transform of sample_inl.h's LogitXf.  Every load of a logit goes through it (after
// the raw value has gone to the log-sum-exp, before the temperature and the suppression lists), so every pass sees the same z':
// the logit bias (dtk_set_logit_bias), the presence / frequency penalty with the id's count, the DRY penalty with the id's match length
// (dtk_set_dry; k_dry_scan leaves the lengths in front of this kernel) and the EOS rules of the sequence's length
// (dtk_set_length_control), each behind a block-uniform test: a sequence without the value reads nothing of its table.  The sampled token
// goes to pen_tok (sample_commit) for k_count_token, which runs behind this kernel: no block reads the tables after its update.
// PN = false is the kernel as it was before the penalties existed.
template <bool LP, bool TR, bool PN>
__global__ __launch_bounds__(SAMPLE_THREADS) void k_sample(SampleArgs a) {
  if (!sample_bind_slot<PN>(a, blockIdx.x)) return;      // batched decode: one block per slot, same code on that slot's buffers
  __shared__ float s_f[16];
  __shared__ int s_i[16];
  __shared__ unsigned long long s_q[16];
  __shared__ unsigned long long h_mass[256];
  __shared__ unsigned int h_cnt[256];
  __shared__ unsigned long long sc_above_q;
  __shared__ unsigned int sc_above_c;
  __shared__ unsigned int sc_prefix;
  __shared__ unsigned int sc_bin;
  __shared__ unsigned long long scan[SAMPLE_THREADS];
  __shared__ int s_token;
  __shared__ float s_max;
  __shared__ unsigned long long s_total;
  __shared__ float s_lm[16], s_ls[16];     // LP: the waves' log-sum-exp states
  __shared__ unsigned long long s_tokq;    // LP: the chosen token's integer mass, published by the thread that chose it

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.V;
  // the sampling configuration is read once into LDS (is_banned runs for every vocabulary entry)
  __shared__ SamplingDev s_sp;
  if (tid < (int)(sizeof(SamplingDev) / 4)) reinterpret_cast<uint32_t*>(&s_sp)[tid] = reinterpret_cast<const uint32_t*>(a.sp)[tid];
  __syncthreads();
  const SamplingDev* sp = &s_sp;
  const uint32_t draw = (a.step_override >= 0) ? (uint32_t)a.step_override : a.st->draw;
  const int forced = a.advance ? a.st->force_plus1 : 0;
  const bool first = (draw == 0);
  const bool sampling = sp->do_sample != 0;
  const float invT = sampling ? 1.f / sp->temperature : 1.f;
  LogitXf xf;                                         // PN: the sequence's transform (block-uniform)
  xf.bind<PN>(a, sample_cur<PN>(a));

  // ---- pass 1: masked (scaled) max and first argmax.  16-byte loads, four per thread in flight
  // (the greedy path is one memory round trip + the block reduction)
  float best = -INFINITY;
  int besti = 0x7fffffff;
  float lm = -INFINITY, ls = 0.f;
  const bool vec = ((V & 3) == 0) && ((reinterpret_cast<uintptr_t>(a.logits) & 15) == 0);
  if (vec) {
    const int V4 = V >> 2;
    const f32x4* l4 = reinterpret_cast<const f32x4*>(a.logits);
    for (int base = tid; base < V4; base += 4 * SAMPLE_THREADS) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i4 = base + u * SAMPLE_THREADS;
        v[u] = (i4 < V4) ? l4[i4] : (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i4 = base + u * SAMPLE_THREADS;
        if (i4 >= V4) continue;
        if constexpr (LP) {
#pragma unroll
          for (int e = 0; e < 4; ++e) lse_push(lm, ls, v[u][e]);
        }
        if constexpr (PN) xf.vec<4>(a, i4 * 4, v[u]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = i4 * 4 + e;
          float z = v[u][e] * invT;
          if (is_banned(sp, i, first)) z = -INFINITY;
          if (z > best || (z == best && i < besti)) { best = z; besti = i; }
        }
      }
    }
  } else {
    for (int i = tid; i < V; i += SAMPLE_THREADS) {
      float z = a.logits[i];
      if constexpr (LP) lse_push(lm, ls, z);
      if constexpr (PN) z = xf.one(a, i, z);
      z *= invT;
      if (is_banned(sp, i, first)) z = -INFINITY;
      if (z > best || (z == best && i < besti)) { best = z; besti = i; }
    }
  }
  if constexpr (LP) { lse_wave(lm, ls); if (lane == 0) { s_lm[wave] = lm; s_ls[wave] = ls; } }
  block_argmax_first<SAMPLE_THREADS>(best, besti, s_f, s_i);
  if (tid == 0) {
    s_max = best; s_token = besti;
    if constexpr (LP) {      // thread 0 holds wave 0's state: fold the others in wave order
      for (int w = 1; w < 16; ++w) lse_merge(lm, ls, s_lm[w], s_ls[w]);
    }
  }
  __syncthreads();
  const float zmax = s_max;
  const int amax = s_token;                      // TR: the fallback's survivor (the draw overwrites s_token)
  (void)amax;
  unsigned long long lp_q = 0, lp_total = 1;     // LP, thread 0: the chosen token's integer mass and the kept set's

  if (sampling) {
    // fixed-point mass q_i = floor(exp(z_i - zmax) * 2^31)  (fits 32 bits; exact integer sums)
    auto mass = [&](int i, float& z) -> unsigned long long {
      z = a.logits[i];
      if constexpr (PN) z = xf.one(a, i, z);
      z *= invT;
      if (is_banned(sp, i, first)) z = -INFINITY;
      const float e = expf(z - zmax);
      return (unsigned long long)((double)e * 2147483648.0);
    };
    // ---- radix descent for the keep-threshold key.  Top-k then top-p, as HF orders the
    // warpers: top-k keeps keys >= (k-th largest); top-p then works on the softmax of the
    // survivors: keep token iff the mass strictly above it is < top_p * total.
    uint32_t thr_k = 0;  // keep keys >= thr_k
    if (sp->top_k > 0 && sp->top_k < V) {
      uint32_t prefix = 0; unsigned int above = 0;
      for (int level = 3; level >= 0; --level) {
        const int shift = level * 8;
        for (int b = tid; b < 256; b += SAMPLE_THREADS) h_cnt[b] = 0;
        __syncthreads();
        for (int i = tid; i < V; i += SAMPLE_THREADS) {
          float z; (void)mass(i, z);
          const uint32_t key = fkey(z);
          const bool match = (level == 3) || ((key >> (shift + 8)) == (prefix >> (shift + 8)));
          if (match) atomicAdd(&h_cnt[(key >> shift) & 255], 1u);
        }
        __syncthreads();
        if (tid == 0) {
          unsigned int ab = above; int bsel = 0;
          for (int b = 255; b >= 0; --b) {
            if (h_cnt[b] == 0) continue;
            if (ab + h_cnt[b] >= (unsigned)sp->top_k) { bsel = b; break; }
            ab += h_cnt[b];
          }
          sc_above_c = ab; sc_bin = bsel;
        }
        __syncthreads();
        above = sc_above_c;
        prefix |= (sc_bin << shift);
        __syncthreads();
      }
      thr_k = prefix;
    }
    // total mass of top-k survivors
    unsigned long long loc = 0;
    for (int i = tid; i < V; i += SAMPLE_THREADS) {
      float z; const unsigned long long q = mass(i, z);
      if (fkey(z) >= thr_k) loc += q;
    }
    loc = block_sum_u64<SAMPLE_THREADS>(loc, s_q);
    if (tid == 0) s_total = loc;
    __syncthreads();
    const unsigned long long total_k = s_total;

    uint32_t thr = thr_k;
    if (sp->top_p < 1.0f) {
      const unsigned long long pq = (unsigned long long)((double)sp->top_p * (double)total_k);
      uint32_t prefix = 0; unsigned long long above = 0;
      for (int level = 3; level >= 0; --level) {
        const int shift = level * 8;
        for (int b = tid; b < 256; b += SAMPLE_THREADS) { h_mass[b] = 0; h_cnt[b] = 0; }
        __syncthreads();
        for (int i = tid; i < V; i += SAMPLE_THREADS) {
          float z; const unsigned long long q = mass(i, z);
          const uint32_t key = fkey(z);
          if (key < thr_k) continue;
          const bool match = (level == 3) || ((key >> (shift + 8)) == (prefix >> (shift + 8)));
          if (match) {
            atomicAdd(&h_mass[(key >> shift) & 255], q);
            atomicAdd(&h_cnt[(key >> shift) & 255], 1u);
          }
        }
        __syncthreads();
        if (tid == 0) {
          // lowest non-empty bin whose strictly-above mass is still < pq
          unsigned long long ab = above; int bsel = -1; unsigned long long ab_sel = above;
          for (int b = 255; b >= 0; --b) {
            if (h_cnt[b] == 0) continue;
            if (ab < pq || bsel < 0) { bsel = b; ab_sel = ab; } else break;
            ab += h_mass[b];
          }
          sc_above_q = ab_sel; sc_bin = (unsigned)bsel;
        }
        __syncthreads();
        above = sc_above_q;
        prefix |= (sc_bin << shift);
        __syncthreads();
      }
      thr = prefix > thr_k ? prefix : thr_k;
    }
    // ---- TR: the mass floor of min-p and epsilon
    uint32_t qfl = 0; bool fb = false;
    if constexpr (TR) {
      unsigned long long total_m = 0;      // the mass kept behind top-p and min-p: read by epsilon alone
      if (sp->eps > 0.f) {      // block-uniform
        const unsigned long long fl = (unsigned long long)sp->qmin;
        unsigned long long pre = 0;
        for (int i = tid; i < V; i += SAMPLE_THREADS) {
          float z; const unsigned long long q = mass(i, z);
          if (fkey(z) >= thr && q >= fl) pre += q;
        }
        pre = block_sum_u64<SAMPLE_THREADS>(pre, s_q);
        if (tid == 0) s_total = pre;
        __syncthreads();
        total_m = s_total;
      }
      trunc_floor(sp->qmin, sp->eps, total_m, qfl, fb);
    }
    auto kept_el = [&](int i, float z, unsigned long long q) -> bool { return sample_kept<TR>(fkey(z), (uint32_t)q, i, thr, qfl, fb, amax); };
    // ---- kept mass + inverse-CDF draw in index order
    const int per = (V + SAMPLE_THREADS - 1) / SAMPLE_THREADS;
    const int i0 = tid * per, i1 = min(V, i0 + per);
    unsigned long long mine = 0;
    for (int i = i0; i < i1; ++i) {
      float z; const unsigned long long q = mass(i, z);
      if (kept_el(i, z, q)) mine += q;
    }
    block_scan_u64<SAMPLE_THREADS>(scan, mine);
    const unsigned long long kept = scan[SAMPLE_THREADS - 1];
    const unsigned long long target = draw_target(sp->seed, draw, kept);
    const unsigned long long excl = scan[tid] - mine;
    if (mine > 0 && target >= excl && target < excl + mine) {
      unsigned long long run = excl;
      for (int i = i0; i < i1; ++i) {
        float z; const unsigned long long q = mass(i, z);
        if (kept_el(i, z, q)) {
          if (target < run + q) { s_token = i; if constexpr (LP) s_tokq = q; break; }
          run += q;
        }
      }
    }
    if (a.probs_out) {
      for (int i = tid; i < V; i += SAMPLE_THREADS) {
        float z; const unsigned long long q = mass(i, z);
        a.probs_out[i] = kept_el(i, z, q) ? (float)((double)q / (double)kept) : 0.f;
      }
    }
    __syncthreads();
    if constexpr (LP) if (tid == 0) { lp_q = s_tokq; lp_total = kept; }
  } else if (a.probs_out) {
    for (int i = tid; i < V; i += SAMPLE_THREADS) a.probs_out[i] = (i == s_token) ? 1.f : 0.f;
  }

  float2 lp = make_float2(0.f, 0.f); float lse = 0.f;      // LP, thread 0: against the block's log-sum-exp state of the raw row
  if constexpr (LP) if (tid == 0 && forced <= 0) { lp = lp_pair(a.logits[s_token], lm, ls, sampling, lp_q, lp_total); lse = lm + logf(ls); }
  sample_commit<LP, PN, SAMPLE_THREADS>(a, s_token, forced, draw, lp, lse);
}

// ------------------------------------------------------------------------------------------
// Register-resident sampler for vocabularies up to 32 768 (every v1 model): thread t owns the 32
// CONSECUTIVE logits [32t, 32t+32) — one 128-byte line, read once with 16-byte loads — and keeps their keys
// and integer masses in registers through every pass (argmax, top-k / top-p radix descent, inverse-CDF
// scan), so the whole sampler is ONE pass over the logits.  Histogram updates are run-length
// aggregated per thread (neighbouring logits mostly share the high key byte), which removes the
// same-address LDS-atomic serialisation that dominated k_sample (190 us -> measured in profiles/).
// Same integer semantics as k_sample / oracle/sampling.py (bit-exact kept set and draws).
// LP as in k_sample: the raw logits are in registers before the temperature is applied, so the thread's log-sum-exp state is their
// maximum and one expf per logit.  TR as in k_sample: the mass floor is one more walk over the 32 keys and one block reduction.
// PN as in k_sample: the thread's 32 counts are one 64-byte line, read as 8-byte words beside the 16-byte loads of the logits.
#define SF_PER 32
template <bool LP, bool TR, bool PN>
__global__ __launch_bounds__(SAMPLE_THREADS) void k_sample_fast(SampleArgs a) {
  if (!sample_bind_slot<PN>(a, blockIdx.x)) return;
  __shared__ SamplingDev s_sp;
  __shared__ float s_f[16];
  __shared__ int s_i[16];
  __shared__ unsigned long long s_q[16];
  __shared__ unsigned long long h_mass[256];
  __shared__ unsigned int h_cnt[256];
  __shared__ unsigned long long sc_above_q;
  __shared__ unsigned int sc_above_c, sc_bin;
  __shared__ unsigned long long scan[SAMPLE_THREADS];
  __shared__ int s_token;
  __shared__ float s_max;
  __shared__ unsigned long long s_total;
  __shared__ unsigned long long s_bw[8];
  __shared__ int s_bi[8];
  __shared__ float s_lm[16], s_ls[16];     // LP: the waves' log-sum-exp states
  __shared__ unsigned long long s_tokq;    // LP: the chosen token's integer mass, published by the thread that chose it
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.V;
  if (tid < (int)(sizeof(SamplingDev) / 4)) reinterpret_cast<uint32_t*>(&s_sp)[tid] = reinterpret_cast<const uint32_t*>(a.sp)[tid];
  __syncthreads();
  const SamplingDev* sp = &s_sp;
  const uint32_t draw = (a.step_override >= 0) ? (uint32_t)a.step_override : a.st->draw;
  const int forced = a.advance ? a.st->force_plus1 : 0;
  const bool first = (draw == 0);
  const bool sampling = sp->do_sample != 0;
  const float invT = sampling ? 1.f / sp->temperature : 1.f;
  LogitXf xf;                                         // PN: the sequence's transform (block-uniform)
  xf.bind<PN>(a, sample_cur<PN>(a));
  const int i0 = tid * SF_PER;

  // ---- the one pass over the logits
  float z[SF_PER];
  float lm = -INFINITY, ls = 0.f;
  const bool vec = ((reinterpret_cast<uintptr_t>(a.logits) & 15) == 0) && (i0 + SF_PER <= V);
  if constexpr (LP) {     // the same loads; every 16-byte load is folded into the log-sum-exp state before the temperature is applied
    if (vec) {
      const f32x4* l4 = reinterpret_cast<const f32x4*>(a.logits + i0);
#pragma unroll
      for (int k = 0; k < SF_PER / 4; ++k) {
        f32x4 v = l4[k];
        const float m4 = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
        if (m4 > lm) { ls *= expf(lm - m4); lm = m4; }
        ls += (expf(v[0] - lm) + expf(v[1] - lm)) + (expf(v[2] - lm) + expf(v[3] - lm));
        if constexpr (PN) xf.vec<4>(a, i0 + 4 * k, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) z[4 * k + e] = v[e] * invT;
      }
    } else {
#pragma unroll
      for (int k = 0; k < SF_PER; ++k) {
        float v = (i0 + k < V) ? a.logits[i0 + k] : -INFINITY;
        lse_push(lm, ls, v);
        if constexpr (PN) if (i0 + k < V) v = xf.one(a, i0 + k, v);
        z[k] = v * invT;
      }
    }
  } else if (vec) {
    const f32x4* l4 = reinterpret_cast<const f32x4*>(a.logits + i0);
#pragma unroll
    for (int k = 0; k < SF_PER / 4; ++k) {
      f32x4 v = l4[k];
      if constexpr (PN) xf.vec<4>(a, i0 + 4 * k, v);
#pragma unroll
      for (int e = 0; e < 4; ++e) z[4 * k + e] = v[e] * invT;
    }
  } else if constexpr (PN) {
#pragma unroll
    for (int k = 0; k < SF_PER; ++k)
      z[k] = (i0 + k < V) ? xf.one(a, i0 + k, a.logits[i0 + k]) * invT : -INFINITY;
  } else {
#pragma unroll
    for (int k = 0; k < SF_PER; ++k) z[k] = (i0 + k < V) ? a.logits[i0 + k] * invT : -INFINITY;
  }
  // bans: a handful of ids, each owned by exactly one thread (static register index via the unrolled compare)
  {
    const int nb = sp->n_bad, na = sp->n_always, ng = first ? sp->n_begin : 0;
    for (int j = 0; j < nb + na + ng; ++j) {
      const int id = j < nb ? sp->bad_ids[j] : (j < nb + na ? sp->always_ids[j - nb] : sp->begin_ids[j - nb - na]);
      const int rel = id - i0;
      if (rel >= 0 && rel < SF_PER) {
#pragma unroll
        for (int k = 0; k < SF_PER; ++k) if (k == rel) z[k] = -INFINITY;
      }
    }
  }
  float best = -INFINITY;
  int besti = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < SF_PER; ++k)
    if (i0 + k < V && (z[k] > best || (z[k] == best && i0 + k < besti))) { best = z[k]; besti = i0 + k; }
  if constexpr (LP) { lse_wave(lm, ls); if (lane == 0) { s_lm[wave] = lm; s_ls[wave] = ls; } }
  block_argmax_first<SAMPLE_THREADS>(best, besti, s_f, s_i);
  if (tid == 0) {
    s_max = best; s_token = besti;
    if constexpr (LP) {      // thread 0 holds wave 0's state: fold the others in wave order
      for (int w = 1; w < 16; ++w) lse_merge(lm, ls, s_lm[w], s_ls[w]);
    }
  }
  __syncthreads();
  const float zmax = s_max;
  const int amax = s_token;                      // TR: the fallback's survivor (the draw overwrites s_token)
  (void)amax;
  unsigned long long lp_q = 0, lp_total = 1;     // LP, thread 0: the chosen token's integer mass and the kept set's

  if (sampling) {
    // integer mass floor(exp(z - zmax) * 2^31) <= 2^31 of logit k.  Recomputed from the key wherever it is needed (the key is an
    // invertible image of the logit, so the value is the same every time): holding 32 masses next to 32 keys put the kernel 33
    // VGPRs + 201 SGPRs over the 128-register budget of a 1024-thread block (profiles/r03_kernel_resources.txt: 136 B of scratch)
#pragma unroll
    for (int k = 0; k < SF_PER; ++k) {
      const bool in = i0 + k < V;
      z[k] = __uint_as_float(in ? fkey(z[k]) : 0u);   // the slot now holds the order-preserving key
    }
#define key(k) __float_as_uint(z[k])
    auto mass_of = [&](uint32_t kb) -> uint32_t {     // only called for k with i0 + k < V
      const float zz = (kb & 0x80000000u) ? __uint_as_float(kb & 0x7fffffffu) : __uint_as_float(~kb);
      return (uint32_t)((double)expf(zz - zmax) * 2147483648.0);
    };
#define q_(k) mass_of(key(k))
    // radix descent helper state: run-length aggregated histogram update
    uint32_t thr_k = 0;
    if (sp->top_k > 0 && sp->top_k < V) {
      uint32_t prefix = 0; unsigned int above = 0;
      for (int level = 3; level >= 0; --level) {
        const int shift = level * 8;
        for (int b = tid; b < 256; b += SAMPLE_THREADS) h_cnt[b] = 0;
        __syncthreads();
        uint32_t cur = 0xffffffffu, cc = 0;
#pragma unroll
        for (int k = 0; k < SF_PER; ++k) {
          if (i0 + k >= V) continue;
          const bool match = (level == 3) || ((key(k) >> (shift + 8)) == (prefix >> (shift + 8)));
          if (!match) continue;
          const uint32_t bin = (key(k) >> shift) & 255u;
          if (bin != cur) { if (cc) atomicAdd(&h_cnt[cur], cc); cur = bin; cc = 0; }
          ++cc;
        }
        if (cc) atomicAdd(&h_cnt[cur], cc);
        __syncthreads();
        if (tid == 0) {
          unsigned int ab = above; int bsel = 0;
          for (int b = 255; b >= 0; --b) {
            if (h_cnt[b] == 0) continue;
            if (ab + h_cnt[b] >= (unsigned)sp->top_k) { bsel = b; break; }
            ab += h_cnt[b];
          }
          sc_above_c = ab; sc_bin = bsel;
        }
        __syncthreads();
        above = sc_above_c;
        prefix |= (sc_bin << shift);
        __syncthreads();
      }
      thr_k = prefix;
    }
    unsigned long long loc = 0;
#pragma unroll
    for (int k = 0; k < SF_PER; ++k) if (i0 + k < V && key(k) >= thr_k) loc += q_(k);
    loc = block_sum_u64<SAMPLE_THREADS>(loc, s_q);
    if (tid == 0) s_total = loc;
    __syncthreads();
    const unsigned long long total_k = s_total;

    uint32_t thr = thr_k;
    if (sp->top_p < 1.0f) {
      const unsigned long long pq = (unsigned long long)((double)sp->top_p * (double)total_k);
      uint32_t prefix = 0; unsigned long long above = 0;
      for (int level = 3; level >= 0; --level) {
        const int shift = level * 8;
        for (int b = tid; b < 256; b += SAMPLE_THREADS) { h_mass[b] = 0; h_cnt[b] = 0; }
        __syncthreads();
        uint32_t cur = 0xffffffffu, cc = 0;
        unsigned long long cm = 0;
#pragma unroll
        for (int k = 0; k < SF_PER; ++k) {
          if (i0 + k >= V || key(k) < thr_k) continue;
          const bool match = (level == 3) || ((key(k) >> (shift + 8)) == (prefix >> (shift + 8)));
          if (!match) continue;
          const uint32_t bin = (key(k) >> shift) & 255u;
          if (bin != cur) {
            if (cc) { atomicAdd(&h_mass[cur], cm); atomicAdd(&h_cnt[cur], cc); }
            cur = bin; cc = 0; cm = 0;
          }
          ++cc; cm += q_(k);
        }
        if (cc) { atomicAdd(&h_mass[cur], cm); atomicAdd(&h_cnt[cur], cc); }
        __syncthreads();
        unsigned int bsel; unsigned long long ab_sel;
        bin_select_mass(h_mass, h_cnt, pq, above, s_bw, s_bi, bsel, ab_sel);   // parallel form of the serial 255..0 scan
        above = ab_sel;
        prefix |= (bsel << shift);
      }
      thr = prefix > thr_k ? prefix : thr_k;
    }
    // TR: the mass floor of min-p and epsilon
    uint32_t qfl = 0; bool fb = false;
    if constexpr (TR) {
      unsigned long long total_m = 0;      // the mass kept behind top-p and min-p: read by epsilon alone
      if (sp->eps > 0.f) {      // block-uniform
        const unsigned long long fl = (unsigned long long)sp->qmin;
        unsigned long long pre = 0;
#pragma unroll
        for (int k = 0; k < SF_PER; ++k)
          if (i0 + k < V && key(k) >= thr) { const uint32_t qk = q_(k); if (qk >= fl) pre += qk; }
        // (block_sum_u64 written out: through the helper the two non-LP TR instantiations spill one more register, 52 -> 56 B of scratch)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) pre += __shfl_xor(pre, off, 64);
        if (lane == 0) s_q[wave] = pre;
        __syncthreads();
        if (tid == 0) { unsigned long long t = 0; for (int w = 0; w < 16; ++w) t += s_q[w]; s_total = t; }
        __syncthreads();
        total_m = s_total;
      }
      trunc_floor(sp->qmin, sp->eps, total_m, qfl, fb);
    }
    // element k (i0 + k < V) of the final set; qk = q_(k)
    auto kept_el = [&](int k, uint32_t kb, uint32_t qk) -> bool { return sample_kept<TR>(kb, qk, i0 + k, thr, qfl, fb, amax); };
    // kept mass + inverse-CDF draw in index order (thread t's range is contiguous: a plain block scan)
    unsigned long long mine = 0;
    if constexpr (TR) {
#pragma unroll
      for (int k = 0; k < SF_PER; ++k) if (i0 + k < V && (fb || key(k) >= thr)) { const uint32_t qk = q_(k); if (kept_el(k, key(k), qk)) mine += qk; }
    } else {
#pragma unroll
      for (int k = 0; k < SF_PER; ++k) if (i0 + k < V && key(k) >= thr) mine += q_(k);
    }
    block_scan_u64<SAMPLE_THREADS>(scan, mine);
    const unsigned long long kept = scan[SAMPLE_THREADS - 1];
    const unsigned long long target = draw_target(sp->seed, draw, kept);
    const unsigned long long excl = scan[tid] - mine;
    if (mine > 0 && target >= excl && target < excl + mine) {
      unsigned long long run = excl;
      bool done = false;
#pragma unroll
      for (int k = 0; k < SF_PER; ++k) {
        if (!done && i0 + k < V && (TR ? (fb || key(k) >= thr) : key(k) >= thr)) {
          const unsigned long long qk = q_(k);
          if (TR && !kept_el(k, key(k), (uint32_t)qk)) continue;
          if (target < run + qk) { s_token = i0 + k; done = true; if constexpr (LP) s_tokq = qk; }
          run += qk;
        }
      }
    }
    if (a.probs_out) {
#pragma unroll
      for (int k = 0; k < SF_PER; ++k)
        if (i0 + k < V) a.probs_out[i0 + k] = kept_el(k, key(k), TR ? q_(k) : 0u) ? (float)((double)q_(k) / (double)kept) : 0.f;
    }
    __syncthreads();
    if constexpr (LP) if (tid == 0) { lp_q = s_tokq; lp_total = kept; }
  } else if (a.probs_out) {
#pragma unroll
    for (int k = 0; k < SF_PER; ++k) if (i0 + k < V) a.probs_out[i0 + k] = (i0 + k == s_token) ? 1.f : 0.f;
  }

  float2 lp = make_float2(0.f, 0.f); float lse = 0.f;      // LP, thread 0: against the block's log-sum-exp state of the raw row
  if constexpr (LP) if (tid == 0 && forced <= 0) { lp = lp_pair(a.logits[s_token], lm, ls, sampling, lp_q, lp_total); lse = lm + logf(ls); }
  sample_commit<LP, PN, SAMPLE_THREADS>(a, s_token, forced, draw, lp, lse);
}
#undef key
#undef q_

// dtk_set_option "top_logprobs": the k first entries of the pending RAW logits (no suppression list, no temperature) in the order
// (z descending, id ascending), launched in front of the sampler.  k rounds; a round is the best element strictly behind the previous
// pick: every thread walks its strided share of the row (the row stays in L2 between rounds), a butterfly per wave, the 16 waves' picks
// through LDS.  Exact in any order, so the result does not depend on the thread count.
#define TOP_THREADS 1024
__global__ __launch_bounds__(TOP_THREADS) void k_top_logits(TopArgs a) {
  const float* z = a.logits;
  const DecState* st = a.st;
  TopRec* out;
  if (a.bs) {
    const int slot = blockIdx.x;
    if (!a.bs->active[slot]) return;
    z += (size_t)slot * a.logits_stride;
    st += slot;
    out = a.top_ring + (size_t)((unsigned)a.bs->step % (unsigned)a.ring) * DTK_MAX_BATCH + slot;
  } else out = a.top_ring + st->draw % (uint32_t)a.ring;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (st->force_plus1 > 0) {          // a forced token was not sampled from these (stale) logits
    if (tid < a.k) { out->id[tid] = -1; out->z[tid] = __builtin_nanf(""); }
    return;
  }
  __shared__ float s_z[TOP_THREADS / 64];
  __shared__ int s_i[TOP_THREADS / 64];
  float lz = INFINITY; int lid = -1;
  for (int j = 0; j < a.k; ++j) {
    float bz = -INFINITY; int bi = 0x7fffffff;
    for (int i = tid; i < a.V; i += TOP_THREADS) {
      const float v = z[i];
      if (top_before(lz, lid, v, i) && top_before(v, i, bz, bi)) { bz = v; bi = i; }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float oz = __shfl_xor(bz, off, 64); const int oi = __shfl_xor(bi, off, 64);
      if (top_before(oz, oi, bz, bi)) { bz = oz; bi = oi; }
    }
    if (lane == 0) { s_z[wave] = bz; s_i[wave] = bi; }
    __syncthreads();
    bz = s_z[0]; bi = s_i[0];
#pragma unroll
    for (int w = 1; w < TOP_THREADS / 64; ++w)
      if (top_before(s_z[w], s_i[w], bz, bi)) { bz = s_z[w]; bi = s_i[w]; }
    __syncthreads();
    lz = bz; lid = bi;
    if (tid == 0) { out->id[j] = bi; out->z[j] = bz; }
  }
}
void launch_top_logits(const TopArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_top_logits, dim3(a.bs ? a.nslots : 1), dim3(TOP_THREADS), 0, s, a);
}

static bool sample_fast_ok(const SampleArgs& a) {
  static int force_generic = -1;
  if (force_generic < 0) { const char* e = getenv("DTK_SAMPLER"); force_generic = (e && !strcmp(e, "generic")) ? 1 : 0; }
  return !force_generic && a.V <= SF_PER * SAMPLE_THREADS;
}
void launch_sample(const SampleArgs& a, hipStream_t s) {
  launch_sample_b(a, s);       // a.nslots == 1 without a.bs
}
// a.trunc == 0 (no sequence of this launch has min_p / epsilon_cutoff): the TR = false instantiations, the kernels as they were; a.pen
// == nullptr (none has a presence / frequency penalty): the PN = false ones, likewise
template <bool PN>
static void launch_sample_t(const SampleArgs& a, hipStream_t s) {
  const dim3 g(a.bs ? a.nslots : 1), b(SAMPLE_THREADS);
  const bool fast = sample_fast_ok(a);
  dispatch_lp_tr(a, [&](auto lp, auto tr) {
    constexpr bool LP = decltype(lp)::value, TR = decltype(tr)::value;
    if (fast) hipLaunchKernelGGL((k_sample_fast<LP, TR, PN>), g, b, 0, s, a);
    else hipLaunchKernelGGL((k_sample<LP, TR, PN>), g, b, 0, s, a);
  });
}
void launch_sample_b(const SampleArgs& a, hipStream_t s) {
  if (a.pen) launch_sample_t<true>(a, s); else launch_sample_t<false>(a, s);
}

// dtk_set_penalties: the count tables.  A count is one half of a 32-bit word; both kernels add to the word that holds it (vector
// atomics); a count never reaches 65 536 (max_positions < 65 536, checked where the tables are allocated), so nothing carries over.
__global__ __launch_bounds__(256) void k_count_scatter(const int32_t* ids, int n, uint16_t* cnt, int V) {
  unsigned* w = reinterpret_cast<unsigned*>(cnt);
  for (int i = threadIdx.x; i < n; i += 256) {
    const int t = ids[i];
    if (t >= 0 && t < V) atomicAdd(w + (t >> 1), (t & 1) ? 0x10000u : 1u);
  }
}
// dtk_set_logit_bias: the (id, value) pairs of one sequence into its dense table (val null on the host: the listed ids back to 0, which is
// how a table is cleared).  The pairs travel as kernel arguments (2 KiB), so nothing is staged; plain vector stores, one thread per pair
// (the host refuses a repeated id, so no two threads write one entry)
struct BiasPairs { int32_t ids[DTK_BIAS_MAX]; float val[DTK_BIAS_MAX]; };
__global__ __launch_bounds__(DTK_BIAS_MAX) void k_bias_scatter(BiasPairs p, int n, float* tab, int V) {
  const int i = threadIdx.x;
  if (i >= n) return;
  const int t = p.ids[i];
  if (t >= 0 && t < V) tab[t] = p.val[i];
}
void launch_bias_scatter(const int32_t* ids, const float* val, int n, float* tab, int V, hipStream_t s) {
  if (n <= 0) return;
  if (n > DTK_BIAS_MAX) n = DTK_BIAS_MAX;
  BiasPairs p;
  for (int i = 0; i < DTK_BIAS_MAX; ++i) { p.ids[i] = i < n ? ids[i] : -1; p.val[i] = (i < n && val) ? val[i] : 0.f; }
  hipLaunchKernelGGL(k_bias_scatter, dim3(1), dim3(DTK_BIAS_MAX), 0, s, p, n, tab, V);
}
void launch_count_scatter(const int32_t* ids, int n, uint16_t* cnt, int V, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_count_scatter, dim3(1), dim3(256), 0, s, ids, n, cnt, V);
}
// behind the sampler of a step: thread j takes sequence j's pen_tok (left by the PN sampler: the sampled token, -1 for a forced one),
// counts it where the sequence has penalty values (a sequence without values keeps no table) and appends it to the sequence's DRY
// history where it has a multiplier (d.hist null: a step without DRY); tokens in front of dry_start (DryLen::skip) are not kept
__global__ __launch_bounds__(DTK_MAX_BATCH) void k_count_token(SampleArgs a, DryScanArgs d) {
  const int j = threadIdx.x;
  if (j >= (a.bs ? a.nslots : 1)) return;
  if (a.bs && !a.bs->active[j]) return;
  const int t = a.pen_tok[j];
  if (t < 0) return;
  a.pen_tok[j] = -1;
  if (t >= a.V) return;
  const PenDev p = a.pen[j];
  if (p.pp != 0.f || p.fp != 0.f) {
    unsigned* w = reinterpret_cast<unsigned*>(const_cast<uint16_t*>(a.pen_cnt) + (size_t)j * a.pen_stride);
    atomicAdd(w + (t >> 1), (t & 1) ? 0x10000u : 1u);
  }
  if (d.hist && d.dry[j].on) {
    DryLen l = d.len[j];
    if (l.skip > 0) l.skip--;
    else if (l.n < d.hist_stride) { d.hist[(size_t)j * d.hist_stride + l.n] = t; l.n++; }
    d.len[j] = l;
  }
}
void launch_count_token(const SampleArgs& a, const DryScanArgs& d, hipStream_t s) {
  hipLaunchKernelGGL(k_count_token, dim3(1), dim3(DTK_MAX_BATCH), 0, s, a, d);
}

// ---- DRY (dtk_set_dry): the suffix-match scan in front of the sampler -------------------------------------------------------------
// One block per sequence.  h[0, n) is the history, tail[k] = h[n-1-k].  Position i in [0, n-2] matches when h[i] == tail[0] and h[i+1] is
// no breaker; its length L(i) is 1 + the number of k = 1, 2, ... with i-k >= 0, h[i-k] == tail[k] and tail[k] no breaker, capped at
// DTK_DRY_MAX_MATCH; M[h[i+1]] = max L(i), kept only where it reaches `allowed`.  M is a byte per vocabulary entry; the maximum is taken
// with a compare-and-swap on the word that holds the byte (vector atomics), so the result does not depend on the order of the threads.
// Every id whose byte is set goes to the `touched` list (with repeats: at most one per position), which the NEXT scan of the sequence
// zeroes first: a step clears in O(n), and no entry of one step survives into the next.  Latency-bound (a few thousand compares): the
// scalars, the breakers and the list's length are requested together; the tail needs n, one more round trip.
#define DRY_THREADS 256
__global__ __launch_bounds__(DRY_THREADS) void k_dry_scan(DryScanArgs d) {
  const int q = blockIdx.x, tid = threadIdx.x;
  const int is_active = d.bs ? d.bs->active[q] : 1;
  const DryDev* dv = d.dry + q;
  const int on = dv->on, allowed = dv->allowed, nb = dv->n_brk;
  const int n = d.len[q].n;
  const int nt = d.n_touched[q];
  const int brk = tid < DTK_DRY_MAX_BREAKERS ? dv->brk[tid] : -1;
  if (!is_active || !on) return;      // (block-uniform)
  const int32_t* h = d.hist + (size_t)q * d.hist_stride;
  int32_t* tl = d.touched + (size_t)q * d.hist_stride;
  unsigned* mw = reinterpret_cast<unsigned*>(d.m + (size_t)q * d.m_stride);
  __shared__ int s_tail[DTK_DRY_MAX_MATCH];
  __shared__ int s_tb[DTK_DRY_MAX_MATCH];       // tail[k] is a breaker
  __shared__ int s_brk[DTK_DRY_MAX_BREAKERS];
  __shared__ int s_nt;
  const int tv = (tid < DTK_DRY_MAX_MATCH && tid < n) ? h[n - 1 - tid] : -1;
  for (int i = tid; i < nt; i += DRY_THREADS) {
    const int t = tl[i];
    atomicAnd(mw + (t >> 2), ~(0xffu << ((t & 3) * 8)));
  }
  if (tid < DTK_DRY_MAX_BREAKERS) s_brk[tid] = brk;
  if (tid < DTK_DRY_MAX_MATCH) s_tail[tid] = tv;
  if (tid == 0) s_nt = 0;
  __syncthreads();
  auto is_brk = [&](int t) { bool b = false; for (int j = 0; j < nb; ++j) b = b || s_brk[j] == t; return b; };
  if (tid < DTK_DRY_MAX_MATCH) s_tb[tid] = is_brk(tv) ? 1 : 0;
  __syncthreads();
  if (n < 2 || s_tb[0]) { if (tid == 0) d.n_touched[q] = 0; return; }
  const int last = s_tail[0];
  for (int i = tid; i <= n - 2; i += DRY_THREADS) {
    if (h[i] != last) continue;
    const int t = h[i + 1];
    if (t < 0 || t >= d.V || is_brk(t)) continue;
    int L = 1;
    while (L < DTK_DRY_MAX_MATCH && i - L >= 0 && h[i - L] == s_tail[L] && !s_tb[L]) ++L;
    if (L < allowed) continue;
    unsigned* w = mw + (t >> 2);
    const int sh = (t & 3) * 8;
    unsigned old = atomicOr(w, 0u);      // (the word as the atomics above left it, not a cached copy)
    while (((old >> sh) & 0xffu) < (unsigned)L) {
      const unsigned prev = atomicCAS(w, old, (old & ~(0xffu << sh)) | ((unsigned)L << sh));
      if (prev == old) break;
      old = prev;
    }
    tl[atomicAdd(&s_nt, 1)] = t;
  }
  __syncthreads();
  if (tid == 0) d.n_touched[q] = s_nt;
}
void launch_dry_scan(const DryScanArgs& d, hipStream_t s) {
  hipLaunchKernelGGL(k_dry_scan, dim3(d.nslots), dim3(DRY_THREADS), 0, s, d);
}
