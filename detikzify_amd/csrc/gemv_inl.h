// gemv_inl.h — the streaming core shared by the single-sequence GEMVs (kernels_decode.hip: k_gemv) and the multi-vector GEMVs of
// the <= 4-slot batched step (kernels_decode_mv.hip: k_gemv_mv): a wave owns NR weight rows for the full K, lanes stride K in
// 16-byte chunks (64 lanes x 16 B = 1 KiB per row per load instruction), non-temporal loads straight into VGPRs, two register
// stages, v_dot2c_f32_bf16 against x chunks held in LDS.  A lane folds chunk lane, lane + 64, lane + 128, ... of its row in that
// order whatever U is, so every kernel built on these helpers produces the same fp32 sum for the same (row, x).
#pragma once
#include "common.h"

template <int NR, int U>
__device__ __forceinline__ void gemv_load(u32x4 (&w)[NR][U], const u32x4* (&rows)[NR],
                                          int g, int lane, int K8) {
  if (64 * (g * U + U) <= K8) {  // wave-uniform: the whole group is inside the row -> no predication
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = lane + 64 * (g * U + u);
#pragma unroll
      for (int r = 0; r < NR; ++r) w[r][u] = ld_nt(rows[r] + c);
    }
    return;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int c = lane + 64 * (g * U + u);
    const bool ok = c < K8;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      u32x4 z = {0u, 0u, 0u, 0u};
      w[r][u] = ok ? ld_nt(rows[r] + c) : z;
    }
  }
}

template <int NR, int U>
__device__ __forceinline__ void gemv_fma(float (&acc)[NR], const u32x4 (&w)[NR][U],
                                         const u32x4* xs, int g, int lane, int K8) {
  const bool full = 64 * (g * U + U) <= K8;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int c = lane + 64 * (g * U + u);
    u32x4 xv = {0u, 0u, 0u, 0u};
    if (full || c < K8) xv = xs[c];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = dot8(w[r][u], xv, acc[r]);
  }
}

// fp8 (OCP e4m3) weights: a 16-byte chunk holds 16 weights of one row; they are widened to bf16 pairs
// (exact) and fed to the same v_dot2c_f32_bf16 against 32 bytes of x.  The per-row power-of-two scale is
// applied to the fp32 sum in the epilogue (exact), so the result equals the bf16 kernel on the
// de-quantised ("effective") weights bit for bit at equal accumulation order.
__device__ __forceinline__ float dot16_f8(const u32x4& w, const u32x4& x0, const u32x4& x1, float c) {
  // v_cvt_scalef32_pk_bf16_fp8: two e4m3 bytes -> packed bf16 pair in ONE instruction (exact, scale 1)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bf16x2_t lo = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[j], 1.0f, false);
    const bf16x2_t hi = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[j], 1.0f, true);
    const uint32_t xa = (j < 2) ? x0[2 * j] : x1[2 * j - 4];
    const uint32_t xb = (j < 2) ? x0[2 * j + 1] : x1[2 * j - 3];
    c = __builtin_amdgcn_fdot2_f32_bf16(lo, __builtin_bit_cast(bf16x2_t, xa), c, false);
    c = __builtin_amdgcn_fdot2_f32_bf16(hi, __builtin_bit_cast(bf16x2_t, xb), c, false);
  }
  return c;
}

template <int NR, int U>
__device__ __forceinline__ void gemv_fma_f8(float (&acc)[NR], const u32x4 (&w)[NR][U],
                                            const u32x4* xs, int g, int lane, int KC) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int c = lane + 64 * (g * U + u);
    u32x4 x0 = {0u, 0u, 0u, 0u}, x1 = {0u, 0u, 0u, 0u};
    if (64 * (g * U + U) <= KC || c < KC) { x0 = xs[2 * c]; x1 = xs[2 * c + 1]; }
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = dot16_f8(w[r][u], x0, x1, acc[r]);
  }
}

// MXFP4 (OCP E2M1 codes + one E8M0 scale per 32 weights along K) weights: a 16-byte chunk c of a row holds the 32 weights
// 32c .. 32c + 31 = exactly one MX block (byte i = weights 2i in the low nibble, 2i + 1 in the high one); its scale is byte c of the
// row's scale array.  v_cvt_scalef32_pk_bf16_fp4 turns two nibbles and the block's power-of-two scale into a packed bf16 pair
// (exact: a 1-bit mantissa times 2^e), so every product is the effective bf16 weight times x and no per-row scale exists.
//
// x for this format lies in LDS in a swizzled order.  A lane's chunk multiplies against the 64 bytes xs[4c .. 4c + 3]; stored
// linearly, the 16 lanes of a ds_read_b128 group would stride 64 bytes and share 4 of the 16 slots of the 256-byte bank row
// (4-way).  So every 1 KiB of x (64 16-byte pieces q = 4c + j) is stored transposed: piece j of the 16 chunks c & 15 forms one
// bank row, chunk c in slot (c & 15) ^ 2j.  The four lane groups of a ds_read_b128 ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and
// the same + 32) each hold 16 lanes with 16 distinct lane & 15, hence 16 distinct c & 15 (c = lane + 64 i); XOR with the constant
// 2j permutes them, so at any j a group reads 16 distinct slots of one bank row: conflict-free by the documented bank rule (not yet
// confirmed with an SQ_LDS_BANK_CONFLICT counter run).  The ^ 2j spreads the prologue's ds_write_b128 (8 consecutive q per group,
// banks mod 32) over 8 distinct slots instead of 2.
__device__ __forceinline__ int f4_xswz(int q) { return (q & ~63) | ((q & 3) << 4) | (((q >> 2) & 15) ^ ((q & 3) << 1)); }
__device__ __forceinline__ int f4_xrows(int KC) { return (4 * KC + 63) & ~63; }   // 16-byte pieces of the swizzled x (whole 1 KiB tiles)
__device__ __forceinline__ float f4_scale(unsigned e8m0) { return __uint_as_float(e8m0 << 23); }   // 2^(b - 127), b in 1 .. 254 (the quantiser's range)

__device__ __forceinline__ float dot32_f4(const u32x4& w, float sc, const u32x4& x0, const u32x4& x1, const u32x4& x2, const u32x4& x3, float c) {
  // (the x words go through named scalars first, as in dot16_f8: __builtin_bit_cast applied to a vector ELEMENT expression reads element 0)
#define F4_WORD(J, X)                                                                                                           \
  { const uint32_t xa = X[0], xb = X[1], xc = X[2], xd = X[3];                                                                  \
    c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[J], sc, 0), __builtin_bit_cast(bf16x2_t, xa), c, false); \
    c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[J], sc, 1), __builtin_bit_cast(bf16x2_t, xb), c, false); \
    c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[J], sc, 2), __builtin_bit_cast(bf16x2_t, xc), c, false); \
    c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[J], sc, 3), __builtin_bit_cast(bf16x2_t, xd), c, false); }
  F4_WORD(0, x0) F4_WORD(1, x1) F4_WORD(2, x2) F4_WORD(3, x3)
#undef F4_WORD
  return c;
}

// the weights of gemv_load plus each chunk's scale byte (64 consecutive bytes per wave and row: one coalesced load)
template <int NR, int U>
__device__ __forceinline__ void gemv_load_f4(u32x4 (&w)[NR][U], unsigned (&sc)[NR][U], const u32x4* (&rows)[NR], const uint8_t* (&srows)[NR],
                                             int g, int lane, int KC) {
  gemv_load<NR, U>(w, rows, g, lane, KC);
  const bool full = 64 * (g * U + U) <= KC;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int c = lane + 64 * (g * U + u);
#pragma unroll
    for (int r = 0; r < NR; ++r) sc[r][u] = (full || c < KC) ? (unsigned)srows[r][c] : 127u;
  }
}

template <int NR, int U>
__device__ __forceinline__ void gemv_fma_f4(float (&acc)[NR], const u32x4 (&w)[NR][U], const unsigned (&sc)[NR][U],
                                            const u32x4* xs, int g, int lane, int KC) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int c = lane + 64 * (g * U + u);
    u32x4 x0 = {0u, 0u, 0u, 0u}, x1 = x0, x2 = x0, x3 = x0;
    if (64 * (g * U + U) <= KC || c < KC) {
      const int b = ((c >> 4) << 6) | (c & 15);          // f4_xswz(4c + j) = b + 16j with the slot ^ 2j
      x0 = xs[b]; x1 = xs[(b + 16) ^ 2]; x2 = xs[(b + 32) ^ 4]; x3 = xs[(b + 48) ^ 6];
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = dot32_f4(w[r][u], f4_scale(sc[r][u]), x0, x1, x2, x3, acc[r]);
  }
}
