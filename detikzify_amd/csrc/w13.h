// w13.h — bf16 weight rows as exact 13-bit planes (the single-sequence decode GEMVs of a bf16 context stream these instead of the
// 16-bit rows; host and device share this file, and it needs nothing but <stdint.h>, so the host code also builds stand-alone).
//
// A bf16 is sign | 8-bit exponent field e | 7-bit mantissa.  Per row one byte hb = max over the row of e >> 1, and the decode base
// lo = max(hb - 15, 0).  Per weight:
//   L, 8 bits: the raw low byte (e & 1, then the mantissa);
//   N, 4 bits: code = (e >> 1) - lo for e >> 1 in [lo + 1, hb] (1 .. 15); code 0 = "e >> 1 is 0" (+-0, denormals, e = 1: the low byte
//              carries e & 1 and the mantissa, so they stay exact).  With lo = 0 the code is e >> 1 itself and the two rules coincide;
//   S, 1 bit : the sign.
// Decode: high byte = S << 7 | (code ? lo + code : 0); weight = high byte || L.  Exact for every pattern whose e >> 1 is 0 or inside
// the row's window [hb - 14, hb] (15 values of e >> 1 = 30 binades; Inf / NaN are patterns like any other: e >> 1 = 127).  A row with
// a weight below the window is UNPACKABLE: w13_pack_row says so and the caller keeps the bf16 row.
//
// Layout of one row (K a multiple of 8; chunk c = the 8 weights 8c .. 8c + 7, as in gemv_inl.h; a lane of the GEMV folds chunks
// lane, lane + 64, ...): a UNIT is two k-iterations = 128 chunks, a sign BLOCK four = 256 chunks.  With J2 = ceil(K / 1024) units and
// J4 = ceil(J2 / 2) blocks the row is [L plane: J2 KiB][N plane: J2 x 512 B][S plane: J4 x 256 B], every plane 16-byte aligned:
//   L: unit j, lane l -> 16 bytes at (64 j + l) * 16: the low bytes of chunk 128 j + l, then those of chunk 128 j + 64 + l  (dwordx4)
//   N: unit j, lane l ->  8 bytes at (64 j + l) * 8: one dword per chunk; byte k = weight k (low nibble), weight 4 + k (high)  (dwordx2)
//   S: block b, lane l -> one dword at (64 b + l) * 4: GROUP g = 2 i + h is the half h (weights 4 h .. 4 h + 3) of the chunk of
//      k-iteration i = 0 .. 3 of the block (chunk 256 b + 64 i + l); the sign of weight k of group g is bit 8 k + g              (dword)
// so the four codes of a group are the bytes of (N >> 4 h) & 0x0f0f0f0f and their signs the bits 7 of the bytes of S << (7 - g).
// Chunks behind the row's end hold zero in every plane (code 0, L 0 = +0).  K = 4096: 6656 B (13 / 16 of 8192); K = 11008: 18432.
//
// The row byte on the DEVICE is hb | W13_ZROW: hb <= 127, and its free top bit says that some weight of the row (inside K, the padding
// does not count) has code 0, i.e. e >> 1 == 0.  In a row without the bit every code is 1 .. 15, so the high byte is lo + code without
// the "code ?" (w13_high_nz): the kernels decode such rows in fewer operations and take the general rule (w13_high) for the others.
// Behind the row's end the short rule gives lo << 8, a finite value that only ever meets x = 0.  The host packer's *hb stays plain hb;
// w13_row_byte is the device's byte, and w13_lo takes either.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define W13_HD __host__ __device__
#else
#define W13_HD
#endif

W13_HD static inline int w13_units(int K) { return ((K >> 3) + 127) >> 7; }
W13_HD static inline int w13_blocks(int K) { return (w13_units(K) + 1) >> 1; }
W13_HD static inline size_t w13_n_off(int K) { return (size_t)w13_units(K) * 1024; }
W13_HD static inline size_t w13_s_off(int K) { return (size_t)w13_units(K) * 1536; }
W13_HD static inline size_t w13_row_bytes(int K) { return (size_t)w13_units(K) * 1536 + (size_t)w13_blocks(K) * 256; }
#define W13_ZROW 0x80   // device row byte: some weight of the row has code 0
W13_HD static inline int w13_lo(int hb) { hb &= 0x7f; return hb > 15 ? hb - 15 : 0; }   // hb, or the device's row byte
// the exponent part of the high byte: any row, and a row without W13_ZROW (no code is 0)
W13_HD static inline int w13_high(int code, int lo) { return code ? lo + code : 0; }
W13_HD static inline int w13_high_nz(int code, int lo) { return lo + code; }

// where weight k of a row lies: byte offsets into the row, the nibble's shift and the sign's bit inside its byte
struct W13Pos { size_t l, n, s; int nshift, sbit; };
W13_HD static inline W13Pos w13_pos(int K, int k) {
  const int c = k >> 3, e = k & 7, lane = c & 63;
  W13Pos p;
  p.l = (size_t)((c >> 7) * 64 + lane) * 16 + (size_t)(((c >> 6) & 1) * 8 + e);
  p.n = w13_n_off(K) + (size_t)((c >> 7) * 64 + lane) * 8 + (size_t)(((c >> 6) & 1) * 4 + (e & 3));
  p.nshift = (e >> 2) * 4;
  p.s = w13_s_off(K) + (size_t)((c >> 8) * 64 + lane) * 4 + (size_t)(e & 3);
  p.sbit = 2 * ((c >> 6) & 3) + (e >> 2);
  return p;
}

// the row's hb byte
static inline int w13_row_hb(const uint16_t* w, int K) {
  int hb = 0;
  for (int k = 0; k < K; ++k) { const int q = (w[k] >> 8) & 0x7f; if (q > hb) hb = q; }
  return hb;
}
// the device's row byte: hb, and W13_ZROW if a weight of the row has e >> 1 == 0 (+-0, a denormal, e = 1)
static inline int w13_row_byte(const uint16_t* w, int K) {
  int z = 0;
  for (int k = 0; k < K; ++k) if (((w[k] >> 8) & 0x7f) == 0) z = W13_ZROW;
  return w13_row_hb(w, K) | z;
}
// code of one weight under decode base lo, or -1: below the window
W13_HD static inline int w13_code(unsigned w, int lo) {
  const int q = (int)((w >> 8) & 0x7fu);
  if (q == 0) return 0;
  return q > lo ? q - lo : -1;
}
// Pack one row into `row` (w13_row_bytes(K) bytes, overwritten) and *hb.  Returns the number of weights below the window: 0 = packed;
// otherwise the row is unpackable and `row` holds zeros for those weights (never a silently altered value the caller could stream:
// the caller must drop the row).
static inline int w13_pack_row(const uint16_t* w, int K, uint8_t* row, uint8_t* hb_out) {
  const int hb = w13_row_hb(w, K), lo = w13_lo(hb);
  int bad = 0;
  const size_t nb = w13_row_bytes(K);
  for (size_t i = 0; i < nb; ++i) row[i] = 0;
  for (int k = 0; k < K; ++k) {
    const int code = w13_code(w[k], lo);
    if (code < 0) { ++bad; continue; }
    const W13Pos p = w13_pos(K, k);
    row[p.l] = (uint8_t)(w[k] & 0xff);
    row[p.n] = (uint8_t)(row[p.n] | (code << p.nshift));
    row[p.s] = (uint8_t)(row[p.s] | (((w[k] >> 15) & 1) << p.sbit));
  }
  *hb_out = (uint8_t)hb;
  return bad;
}
// hb: the row's hb or the device's row byte
static inline void w13_unpack_row(const uint8_t* row, int hb, int K, uint16_t* w) {
  const int lo = w13_lo(hb);
  for (int k = 0; k < K; ++k) {
    const W13Pos p = w13_pos(K, k);
    const int code = (row[p.n] >> p.nshift) & 15, sign = (row[p.s] >> p.sbit) & 1;
    w[k] = (uint16_t)((sign << 15) | (w13_high(code, lo) << 8) | row[p.l]);
  }
}
// the short rule over a whole row: equal to w13_unpack_row exactly when the row's byte has no W13_ZROW
static inline void w13_unpack_row_nz(const uint8_t* row, int hb, int K, uint16_t* w) {
  const int lo = w13_lo(hb);
  for (int k = 0; k < K; ++k) {
    const W13Pos p = w13_pos(K, k);
    const int code = (row[p.n] >> p.nshift) & 15, sign = (row[p.s] >> p.sbit) & 1;
    w[k] = (uint16_t)((sign << 15) | (w13_high_nz(code, lo) << 8) | row[p.l]);
  }
}
