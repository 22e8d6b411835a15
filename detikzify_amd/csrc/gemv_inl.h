// gemv_inl.h — the streaming core shared by the single-sequence GEMVs (kernels_decode.hip: k_gemv) and the multi-vector GEMVs of
// the <= 4-slot batched step (kernels_decode_mv.hip: k_gemv_mv): a wave owns NR weight rows for the full K, lanes stride K in
// 16-byte chunks (64 lanes x 16 B = 1 KiB per row per load instruction), non-temporal loads straight into VGPRs, two register
// stages, v_dot2c_f32_bf16 against x chunks held in LDS.  A lane folds chunk lane, lane + 64, lane + 128, ... of its row in that
// order whatever U is, so every kernel built on these helpers produces the same fp32 sum for the same (row, x).
#pragma once
#include "common.h"
#include "w13.h"

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

// 13-bit planes of a bf16 row (w13.h): a stage is U k-iterations (U a multiple of 4 = whole sign blocks): per row U / 2 dwordx4 of low
// bytes, U / 2 dwordx2 of exponent codes and U / 4 dwords of signs.  The operands rebuilt in registers are the bf16 row's own bits, and
// a lane folds chunk lane, lane + 64, ... with the same four chained v_dot2c_f32_bf16 as gemv_fma, so every fp32 sum equals the bf16
// kernel's.  x lies linearly in LDS as for bf16.  No lane branches on data: the conditions are the wave-uniform "unit inside the row",
// gemv_fma's "chunk inside x" and the caller's choice of NZ, which is uniform too (a wave owns whole rows: k_gemv takes the short decode
// when none of the wave's NR rows has W13_ZROW in its row byte).
typedef __attribute__((ext_vector_type(2))) unsigned short u16x2_t;

// four exponent codes (one per byte, 0 .. 15) -> the four high bytes without their signs: code ? lo + code : 0.  lo2 = lo | lo << 16;
// a byte's "code != 0" is bit 4 of code + 15, and lo + 15 < 256, so the packed 16-bit multiply-add cannot carry between bytes
__device__ __forceinline__ uint32_t w13_high4(uint32_t codes, uint32_t lo2) {
  const uint32_t nz = ((codes + 0x0f0f0f0fu) >> 4) & 0x01010101u;
  const u16x2_t r = __builtin_bit_cast(u16x2_t, nz) * __builtin_bit_cast(u16x2_t, lo2) + __builtin_bit_cast(u16x2_t, codes);
  return __builtin_bit_cast(uint32_t, r);
}

// one chunk: la / lb = the low bytes of weights 0..3 / 4..7, n = the 8 codes, s = the block's sign dword, i = k-iteration in the block,
// lo4 = lo in every byte.  NZ: the row has no code 0 (w13.h: W13_ZROW clear), so the high bytes are codes + lo4 (lo + 15 < 128: no carry
// between bytes) - one v_add where the general rule needs four operations; both rebuild the row's own bits
template <bool NZ>
__device__ __forceinline__ float dot8_w13(uint32_t la, uint32_t lb, uint32_t n, uint32_t s, int i, uint32_t lo4, const u32x4& x, float c) {
  const uint32_t ce = n & 0x0f0f0f0fu, co = (n >> 4) & 0x0f0f0f0fu;
  const uint32_t he = (NZ ? ce + lo4 : w13_high4(ce, lo4 & 0x00ff00ffu)) | ((s << (7 - 2 * i)) & 0x80808080u);
  const uint32_t ho = (NZ ? co + lo4 : w13_high4(co, lo4 & 0x00ff00ffu)) | ((s << (6 - 2 * i)) & 0x80808080u);
  // v_perm_b32: bytes 0..3 of the selector space are the second operand (low bytes), 4..7 the first (high bytes)
  c = dot2(__builtin_amdgcn_perm(he, la, 0x05010400u), x[0], c);
  c = dot2(__builtin_amdgcn_perm(he, la, 0x07030602u), x[1], c);
  c = dot2(__builtin_amdgcn_perm(ho, lb, 0x05010400u), x[2], c);
  c = dot2(__builtin_amdgcn_perm(ho, lb, 0x07030602u), x[3], c);
  return c;
}

template <int NR, int U>
__device__ __forceinline__ void gemv_load_w13(u32x4 (&wl)[NR][U / 2], u32x2 (&wn)[NR][U / 2], uint32_t (&ws)[NR][U / 4],
                                              const u32x4* (&rows)[NR], int g, int lane, int J2, int n_off, int s_off) {
  static_assert(U % 4 == 0, "a stage is whole sign blocks");
  if (2 * (g * (U / 4) + U / 4) <= J2) {   // wave-uniform: every unit of the stage is inside the row -> no predication
#pragma unroll
    for (int ub = 0; ub < U / 4; ++ub) {
      const int b = g * (U / 4) + ub;
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const unsigned char* p = reinterpret_cast<const unsigned char*>(rows[r]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          wl[r][2 * ub + h] = ld_nt(rows[r] + ((2 * b + h) * 64 + lane));
          wn[r][2 * ub + h] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p + n_off) + ((2 * b + h) * 64 + lane));
        }
        ws[r][ub] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p + s_off) + (b * 64 + lane));
      }
    }
    return;
  }
#pragma unroll
  for (int ub = 0; ub < U / 4; ++ub) {
    const int b = g * (U / 4) + ub;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const unsigned char* p = reinterpret_cast<const unsigned char*>(rows[r]);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const bool ok = 2 * b + h < J2;    // rows end on a unit; what lies behind the end decodes to +0
        const u32x4 zl = {0u, 0u, 0u, 0u};
        const u32x2 zn = {0u, 0u};
        wl[r][2 * ub + h] = ok ? ld_nt(rows[r] + ((2 * b + h) * 64 + lane)) : zl;
        wn[r][2 * ub + h] = ok ? __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p + n_off) + ((2 * b + h) * 64 + lane)) : zn;
      }
      ws[r][ub] = (2 * b < J2) ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p + s_off) + (b * 64 + lane)) : 0u;
    }
  }
}

template <int NR, int U, bool NZ>
__device__ __forceinline__ void gemv_fma_w13(float (&acc)[NR], const u32x4 (&wl)[NR][U / 2], const u32x2 (&wn)[NR][U / 2],
                                             const uint32_t (&ws)[NR][U / 4], const uint32_t (&lo4)[NR],
                                             const u32x4* xs, int g, int lane, int K8) {
  const bool full = 64 * (g * U + U) <= K8;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int c = lane + 64 * (g * U + u);
    u32x4 xv = {0u, 0u, 0u, 0u};
    if (full || c < K8) xv = xs[c];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const u32x4& l = wl[r][u >> 1];
      acc[r] = dot8_w13<NZ>((u & 1) ? l[2] : l[0], (u & 1) ? l[3] : l[1], wn[r][u >> 1][u & 1], ws[r][u >> 2], u & 3, lo4[r], xv, acc[r]);
    }
  }
}
