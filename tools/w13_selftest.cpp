// Stand-alone round-trip check of csrc/w13.h's host packer (no GPU, no library): meant to be built with the host sanitizers,
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I detikzify_amd/csrc tools/w13_selftest.cpp -o w13_selftest
// Every buffer is exactly as large as w13.h says, so a wrong offset is a heap overflow the sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "w13.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

// one row of K weights whose e >> 1 lies in [hb - span, hb] (span <= 14: packable), plus `zeros` patterns with e >> 1 == 0
static int check_row(int K, int hb, int span, int zeros, int below) {
  std::vector<uint16_t> w((size_t)K), back((size_t)K);
  for (int k = 0; k < K; ++k) {
    int q = hb - (int)(rnd() % (unsigned)(span + 1));
    if (q < 1) q = 1;
    w[(size_t)k] = (uint16_t)(((rnd() & 1u) << 15) | ((unsigned)q << 8) | (rnd() & 0xffu));
  }
  w[rnd() % (unsigned)K] = (uint16_t)(((rnd() & 1u) << 15) | ((unsigned)hb << 8) | (rnd() & 0xffu));   // the row's maximum is present
  for (int i = 0; i < zeros; ++i) w[rnd() % (unsigned)K] = (uint16_t)(((rnd() & 1u) << 15) | (rnd() & 0xffu));
  int want_bad = 0;
  if (below && hb > 16) {
    const size_t at = (size_t)(rnd() % (unsigned)K);
    if (((w[at] >> 8) & 0x7f) != hb) w[at] = (uint16_t)(((unsigned)(hb - 15) << 8) | 0x55u);
  }
  // the expected outcome from the format's definition, not from w13.h: a weight is below the window iff 0 < e >> 1 < max - 14
  int real_hb = 0;
  for (int k = 0; k < K; ++k) { const int q = (w[(size_t)k] >> 8) & 0x7f; if (q > real_hb) real_hb = q; }
  for (int k = 0; k < K; ++k) { const int q = (w[(size_t)k] >> 8) & 0x7f; want_bad += (q > 0 && q < real_hb - 14); }
  std::vector<uint8_t> row(w13_row_bytes(K));
  uint8_t hbyte = 0;
  const int bad = w13_pack_row(w.data(), K, row.data(), &hbyte);
  if (bad != want_bad || hbyte != real_hb) { std::printf("K %d hb %d: bad %d (want %d), hb byte %d\n", K, hb, bad, want_bad, hbyte); return 1; }
  if (bad) return 0;
  w13_unpack_row(row.data(), hbyte, K, back.data());
  for (int k = 0; k < K; ++k)
    if (back[(size_t)k] != w[(size_t)k]) { std::printf("K %d hb %d: weight %d is %04x, was %04x\n", K, hb, k, back[(size_t)k], w[(size_t)k]); return 1; }
  // the device's row byte, from the format's definition: hb, and W13_ZROW iff a weight has e >> 1 == 0.  The general rule decodes
  // under either byte; the short rule (no "code ?") gives the row exactly when the bit is clear
  int want_z = 0;
  for (int k = 0; k < K; ++k) want_z |= (((w[(size_t)k] >> 8) & 0x7f) == 0) ? W13_ZROW : 0;
  const int byte = w13_row_byte(w.data(), K);
  if (byte != (real_hb | want_z)) { std::printf("K %d hb %d: row byte %02x, want %02x\n", K, hb, byte, real_hb | want_z); return 1; }
  w13_unpack_row(row.data(), byte, K, back.data());
  for (int k = 0; k < K; ++k)
    if (back[(size_t)k] != w[(size_t)k]) { std::printf("K %d row byte %02x: weight %d is %04x, was %04x\n", K, byte, k, back[(size_t)k], w[(size_t)k]); return 1; }
  w13_unpack_row_nz(row.data(), byte, K, back.data());
  int differ = 0;
  for (int k = 0; k < K; ++k) differ += back[(size_t)k] != w[(size_t)k];
  // (with lo == 0 the two rules coincide, so a flagged row may still decode alike: the bit is then merely conservative)
  if (!(byte & W13_ZROW) && differ) { std::printf("K %d row byte %02x: the short rule changes %d weights of an unflagged row\n", K, byte, differ); return 1; }
  if ((byte & W13_ZROW) && w13_lo(byte) > 0 && !differ) { std::printf("K %d row byte %02x: flagged, lo > 0, and the short rule changes nothing\n", K, byte); return 1; }
  return 0;
}

int main() {
  const int Ks[] = {8, 72, 512, 520, 1024, 1032, 1544, 2048, 2056, 11008};
  int fails = 0, rows = 0;
  for (int K : Ks)
    for (int hb = 0; hb <= 127; hb += (hb < 20 || hb > 110) ? 1 : 9)
      for (int span = 0; span <= 14; span += 7)
        for (int zeros = 0; zeros <= 4; zeros += 4)
          for (int below = 0; below <= 1; ++below) { fails += check_row(K, hb, span, zeros, below); ++rows; }
  std::printf("w13 selftest: %d rows, %d failures\n", rows, fails);
  return fails ? 1 : 0;
}
