// common.h — device helpers shared by the gfx950 kernels of libdtk_hip.so.
// wave = 64 lanes everywhere (CDNA4); bf16 values travel as raw uint16 bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

typedef uint16_t bf16_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define DTK_WAVE 64

// Raising a kernel's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) is a per-DEVICE property of the function, so the
// "already done" mark of a launcher is a bit per device, not a process-wide bool: a second dtk_ctx on another GPU of the same process
// sets it again.  A refused attribute is reported once on stderr and remembered (dtk_lds_attr_failed: the step launchers fail on it).
static inline bool dtk_lds_attr_todo(unsigned long long& done) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return true;       // unknown device: set it every time
  const unsigned long long bit = 1ull << dev;
  if (done & bit) return false;
  done |= bit;
  return true;
}
int& dtk_lds_attr_error(int device);                                                // dtk_api.hip: the first hipError_t a launcher's attribute call returned ON THAT DEVICE (0 = none):
                                                                                    // a refusal on one GPU does not fail the contexts of another
static inline void dtk_lds_attr(hipError_t e, const char* file, int line) {
  if (e == hipSuccess) return;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (!dtk_lds_attr_error(dev)) {
    fprintf(stderr, "libdtk_hip: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed on device %d at %s:%d: %s\n", dev, file, line, hipGetErrorString(e));
    dtk_lds_attr_error(dev) = (int)e;
  }
}
#define DTK_LDS_ATTR(call) dtk_lds_attr((call), __FILE__, __LINE__)

__device__ __forceinline__ float bf2f(bf16_t h) { return __uint_as_float(((uint32_t)h) << 16); }
// fp32 -> bf16, round-to-nearest-even (v_cvt_pk_bf16_f32), same as torch .to(bfloat16)
__device__ __forceinline__ bf16_t f2bf(float f) {
  __bf16 h = (__bf16)f;
  return __builtin_bit_cast(unsigned short, h);
}
// round an fp32 value through bf16 (every place HF materialises a bf16 tensor)
__device__ __forceinline__ float rbf(float f) { return bf2f(f2bf(f)); }
__device__ __forceinline__ float pk_lo(uint32_t p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float pk_hi(uint32_t p) { return __uint_as_float(p & 0xffff0000u); }
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  return (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
}
// c + a.lo*b.lo + a.hi*b.hi on packed bf16 pairs, fp32 accumulate (v_dot2c_f32_bf16)
__device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float c) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a),
                                         __builtin_bit_cast(bf16x2_t, b), c, false);
}
__device__ __forceinline__ float dot8(const u32x4& a, const u32x4& b, float c) {
  c = dot2(a[0], b[0], c);
  c = dot2(a[1], b[1], c);
  c = dot2(a[2], b[2], c);
  c = dot2(a[3], b[3], c);
  return c;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
// streamed-once weights: non-temporal 16-byte load
__device__ __forceinline__ u32x4 ld_nt(const u32x4* p) { return __builtin_nontemporal_load(p); }

// Decode-step state that lives in device memory so a captured hipGraph can be
// replayed unchanged: kernels read the position / token from here.
struct DecState {
  int32_t pos;       // position index of the token being forwarded this step
  int32_t next_pos;  // number of tokens that have KV after this step
  int32_t token;     // token sampled this step (input of the forward)
  uint32_t draw;     // number of tokens sampled since dtk_set_sampling
  int32_t force_plus1;   // != 0: this step forwards token force_plus1 - 1 instead of sampling one (dtk_resume_slot); cleared by the sampler
  int32_t pad[3];
};

// Batched decode (kernels_batch_decode.hip): which of the (up to 64) slots take part in this step.
#ifndef DTK_MAX_BATCH
#define DTK_MAX_BATCH 64   // == include/dtk.h
#endif
#ifndef DTK_MAX_TOP
#define DTK_MAX_TOP 8      // == include/dtk.h: the most alternatives per position ("top_logprobs", dtk_score_top)
#endif
// One position's top-k alternatives as the decode step leaves them (dtk_set_option "top_logprobs"): the k first entries of the
// vocabulary ordered by raw logit descending, token id ascending on ties; entries >= k are not written.  A forced token: id -1, z NaN.
struct TopRec { int32_t id[DTK_MAX_TOP]; float z[DTK_MAX_TOP]; };
// (z, id) comes before (bz, bi) in that order
__device__ __forceinline__ bool top_before(float z, int id, float bz, int bi) { return z > bz || (z == bz && id < bi); }
#define DTK_PFX_GRID 16    // group rows of k_attn_prefix_g's grid: row y takes groups y, y + 16, ...
#define DTK_PFX_GROUPS 64  // prefix groups a step can hand to k_attn_prefix_g: the worst case of 64 slots that share nothing (64 singleton groups), so that
                           // whether a slot's prefix goes through the matrix cores never depends on how many OTHER prefixes the step holds (was 16)
// One shared prefix scored on the matrix cores: the active slots that read the first `len` rows of their cache from slot `src`
// (forks of one image: dtk_kv_fork), at most 16 of them = the columns of one MFMA tile.  A source with more forks has several groups.
struct PfxGroup {
  int32_t src;       // the slot whose cache holds the rows
  int32_t len;       // keys [0, len) are the group's shared prefix
  int32_t n;         // members (1..16)
  int32_t pad;
  int32_t slot[16];  // member slots (entries >= n repeat slot[0])
};
struct BatchState {
  int32_t active[DTK_MAX_BATCH];
  int32_t step;      // global step counter (token ring index)
  // Shared prefixes on the matrix cores (k_attn_prefix_g): the host groups the step's active slots by (share_src, share_len) — a
  // property of the slot alone, so whether and how a slot's prefix is scored never depends on which other slots decode with it —
  // into groups of <= 16 slots (at most DTK_PFX_GROUPS = 64: every slot always finds a group); group_plus1[slot] = the slot's group + 1 (0: none, the slot's whole context
  // is walked by k_attn_tail_b).  n_groups == 0: no prefix kernel work this step.
  int32_t n_groups;
  int32_t pad[14];
  // forked slots (dtk_kv_fork) hold a bit-identical copy of their source's first share_len keys: attention reads those
  // rows from the SOURCE slot's cache instead (-1 = none), so the 32 rollouts of one image stream the 243-key image
  // prefix from HBM once per layer and hit the XCD's L2 afterwards
  int32_t share_src[DTK_MAX_BATCH];
  int32_t share_len[DTK_MAX_BATCH];
  int32_t group_plus1[DTK_MAX_BATCH];
  int32_t pfx_len_of[DTK_MAX_BATCH];   // = groups[group_plus1[slot] - 1].len, or 0: what k_attn_tail_b needs, without the dependent lookup
  PfxGroup groups[DTK_PFX_GROUPS];
  // MXFP8 key/value shadow (kv_format "mxfp8"): rows [kv8_from[slot], pos) of the slot were written by decode steps and are read from the
  // shadow planes; rows below it (prefill, fork) exist in bf16 only.  kv8_from[slot] <= pos at every step the slot takes.  Last member:
  // every offset above is what it was.
  int32_t kv8_from[DTK_MAX_BATCH];
};

// Batched decode keeps the GEMV INPUT vectors (normalised x, attention output, SwiGLU activation) of the slots in
// the MFMA B-operand fragment order: tile (slot/16, k/32) is 1 KiB, lane = ((k%32)/8)*16 + slot%16 holds 8
// consecutive k.  A wave's x load is then 1 KiB contiguous (8 full cache lines) instead of 16 rows x 64 B
// (16 half-used lines): measured gate/up at 32 slots 48.3 -> 35.2 us.
__device__ __forceinline__ size_t xtile_off(int slot, int k, int nsteps) {
  return ((size_t)((slot >> 4) * nsteps + (k >> 5)) * 64 + ((k & 31) >> 3) * 16 + (slot & 15)) * 8 + (k & 7);
}

struct SamplingDev {
  int32_t do_sample;
  float temperature;
  float top_p;
  int32_t top_k;
  uint64_t seed;
  int32_t n_bad;
  int32_t bad_ids[8];
  int32_t n_begin;
  int32_t begin_ids[8];
  int32_t n_always;
  int32_t always_ids[8];
  // min-p / epsilon cut-off (dtk_set_sampling_ext; both 0 = off).  Read only by the TR sampler instantiations (SampleArgs::trunc).
  int64_t qmin;          // (int64)((double)min_p * 2^31): the smallest integer mass min-p keeps
  float eps;             // epsilon_cutoff in [0, 1)
};

// presence / frequency penalty of one sequence (dtk_set_penalties; both 0 = off), a record of its own so that SamplingDev keeps its
// tail.  Read only by the PN sampler instantiations (SampleArgs::pen), next to the sequence's uint16 count table.
struct PenDev {
  float pp;              // presence_penalty in [-2, 2]
  float fp;              // frequency_penalty in [-2, 2]
};
// z' of a raw logit z whose id was counted c times: z - (float)((double)pp + (double)fp * c) for c > 0 (the product of a float and an
// integer below 2^16 is exact in double: no contraction can change it), the untouched bits for c = 0
__device__ __forceinline__ float pen_apply(float z, unsigned c, float pp, float fp) {
  return c ? z - (float)((double)pp + (double)fp * (double)c) : z;
}

// DRY (dtk_set_dry; multiplier 0 = off): the penalty of the token that would extend a verbatim repetition of the sequence's own recent
// text.  One record per sequence, read by k_dry_scan (allowed, breakers) and by the PN sampler instantiations (pen) when SampleArgs::dry
// is set.  pen[L] is the host's table (IEEE double, repeated multiplication): no pow runs on the device.
#define DTK_DRY_MAX_MATCH 64
#define DTK_DRY_MAX_BREAKERS 16
struct DryDev {
  float pen[DTK_DRY_MAX_MATCH + 1];   // pen[L] = 0 for L < allowed
  int32_t on;                         // multiplier != 0
  int32_t allowed;                    // dry_allowed_length in [1, 64]
  int32_t n_brk;
  int32_t brk[DTK_DRY_MAX_BREAKERS];  // dry_sequence_breakers
};
// the sequence's history on the device: n ids so far, and how many tokens are still to come before position dry_start is reached
struct DryLen { int32_t n; int32_t skip; };
// z' of a (possibly count-penalised) logit z whose id has match length m in the sequence's table (0: untouched bits; the table holds
// only lengths >= allowed)
__device__ __forceinline__ float dry_apply(float z, unsigned m, const float* pen) { return m ? z - pen[m] : z; }

// Length control and logit bias (dtk_set_length_control / dtk_set_logit_bias; all off by default): a record of its own per sequence,
// read only by the PN sampler instantiations when SampleArgs::len is set.  n = next_pos - start at the sampler.  The EOS rules touch the
// ids eos[0, n_eos): below min_new their logit is -inf; above decay_begin it grows by |z| * m[n - decay_begin], m the sequence's host-built
// table (no pow runs on the device).  n_bias != 0: the sequence's dense float [V] bias table holds something.
#define DTK_BIAS_MAX 256
#define DTK_LEN_MAX_EOS 8
#define DTK_LEN_NO_DECAY 0x7fffffff
struct LenDev {
  int32_t on;                         // an EOS rule can apply: n_eos > 0 and (min_new > 0 or a decay)
  int32_t start;                      // length_start
  int32_t min_new;                    // min_new_tokens
  int32_t decay_begin;                // decay_start, DTK_LEN_NO_DECAY without a decay
  int32_t n_eos;
  int32_t eos[DTK_LEN_MAX_EOS];
  int32_t n_bias;                     // entries of the bias table that are not 0
};
// what a sampler block derives from the record and the sequence's length, once (block-uniform)
struct ShapeRt {
  const float* bias = nullptr;        // the sequence's table, null = no bias
  const int32_t* eos = nullptr;
  int ne = 0;                         // 0 = no EOS rule applies at this length
  float mk = 0.f;                     // m[n - decay_begin]
  bool dec = false, neg = false;      // the decay / the -inf applies
};
__device__ __forceinline__ ShapeRt shape_bind(const LenDev* l, const float* m, const float* bias, int cur) {
  ShapeRt s;
  if (l->n_bias != 0) s.bias = bias;
  if (l->on) {
    const int n = cur - l->start;
    s.neg = n < l->min_new;
    s.dec = n > l->decay_begin;
    if (s.dec) s.mk = m[n - l->decay_begin];
    if (s.neg || s.dec) { s.ne = l->n_eos; s.eos = l->eos; }
  }
  return s;
}
// z + b as one fp32 addition; the untouched bits of z where the table holds 0
__device__ __forceinline__ float bias_apply(float z, float b) { return b != 0.f ? z + b : z; }
// z + fl(|z| * m) in two fp32 roundings.  Contraction is switched off for this body: the build's default would fuse the pair into one fma
// (one rounding), and so would a detour through double, which the compiler narrows back to the fp32 pair first
__device__ __forceinline__ float decay_apply(float z, float m) {
#pragma clang fp contract(off)
  const float p = fabsf(z) * m;
  return z + p;
}
// the EOS rules on the (biased, penalised) logit z of id i: the decay, then -inf
__device__ __forceinline__ float eos_apply(float z, int i, const ShapeRt& s) {
  bool hit = false;
  for (int j = 0; j < s.ne; ++j) hit = hit || s.eos[j] == i;
  if (!hit) return z;
  if (s.dec) z = decay_apply(z, s.mk);
  return s.neg ? -INFINITY : z;
}

// scratch of the multi-block sampler (kernels_sample_mb.hip), one per sequence / slot
#define DTK_SAMPLE_MB_MAX_SLICES 32      // 32 x 8192 = vocabularies up to 262 144
struct SampleMB {
  float bmax[DTK_SAMPLE_MB_MAX_SLICES];
  int32_t barg[DTK_SAMPLE_MB_MAX_SLICES];
  unsigned long long bkept[DTK_SAMPLE_MB_MAX_SLICES];
  unsigned long long hmass[4][256];      // [radix level][bin]: integer probability mass
  unsigned int hcnt[4][256];
  unsigned long long above[4];           // mass strictly above the chosen bin, per level
  unsigned int bin[4];
  unsigned long long total;
  unsigned int thr;
  // DecState.draw / .force_plus1 as they were BEFORE this step's draw kernel (written by block 0 of k_smb_max): k_smb_draw's
  // blocks read only these — its last block rewrites DecState while blocks of the same slot may not have started yet
  unsigned int draw_snap;
  int forced_snap;
  int cur_snap;      // (was padding) DecState.next_pos likewise, written by the PN chain with SampleArgs::len alone: the sequence's length
  // log-probabilities (SampleArgs::lp_ring): every slice's online log-sum-exp state of its RAW logits, left by k_smb_max<true>
  float lmax[DTK_SAMPLE_MB_MAX_SLICES];
  float lsum[DTK_SAMPLE_MB_MAX_SLICES];
  // min-p / epsilon cut-off (SampleArgs::trunc): every slice's mass of the set kept after top-p and min-p, left by k_smb_kept<true>;
  // k_smb_trunc folds them in slice order into the epsilon threshold and publishes the mass floor (or the fallback flag) for k_smb_draw
  unsigned long long bpre[DTK_SAMPLE_MB_MAX_SLICES];
  unsigned int qfl;
  int fb;
};

// Online log-sum-exp over raw logits, carried by the samplers next to their masked maximum (SampleArgs::lp_ring): the state is
// (m, s) = (max so far, sum of exp(z - m)), the identity (-inf, 0).  lse_push takes one logit (one expf), lse_merge folds two states.
// Every sampler applies them in an order fixed by the thread count and V alone, so a row's logsumexp is the same bits every time.
__device__ __forceinline__ void lse_push(float& m, float& s, float z) {
  if (z > m) { s = s * expf(m - z) + 1.f; m = z; }
  else if (m != -INFINITY) s += expf(z - m);
}
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float M = fmaxf(m, om);
  if (M == -INFINITY) { s = 0.f; return; }
  s = s * expf(m - M) + os * expf(om - M);
  m = M;
}
// the block's 16 waves: butterfly inside the wave, lane 0 of every wave to LDS; the caller's thread 0 folds s_m / s_s in wave order
__device__ __forceinline__ void lse_wave(float& m, float& s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float om = __shfl_xor(m, off, 64), os = __shfl_xor(s, off, 64);
    lse_merge(m, s, om, os);
  }
}
// (logprob, sample_logprob) of the delivered token: z_t - lse, and log(q / total) from the sampler's two integers in double
__device__ __forceinline__ float2 lp_pair(float zt, float m, float s, bool sampling, unsigned long long q, unsigned long long total) {
  return make_float2(zt - (m + logf(s)), sampling ? (float)log((double)q / (double)total) : 0.f);
}

// Top-p radix level: among the 256 (mass, count) bins of one level pick the LOWEST non-empty bin whose strictly-above
// mass (above_in + mass of all higher bins) is still < pq; if even the highest non-empty bin fails, pick that one.  This
// is exactly the serial scan `for b = 255..0` of the samplers (whose dependent LDS reads cost ~10 us per level), done by
// threads 0..255 with a wave suffix scan + ballots.  EVERY thread of the block must call it (it contains barriers);
// s_w: 8 x u64 of LDS scratch, s_i: 8 ints.  Results (bin, strictly-above mass of that bin) are returned to all threads.
__device__ __forceinline__ void bin_select_mass(const unsigned long long* s_m, const unsigned int* s_c, unsigned long long pq,
                                                unsigned long long above_in, unsigned long long* s_w, int* s_i,
                                                unsigned int& bin_out, unsigned long long& above_out) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  unsigned long long m = 0, incl = 0; unsigned int c = 0;
  if (tid < 256) {
    m = s_m[tid]; c = s_c[tid];
    incl = m;                                   // inclusive suffix sum over the wave's 64 bins (lanes >= lane)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long v = __shfl_down(incl, off, 64);
      if (lane + off < 64) incl += v;
    }
    if (lane == 0) s_w[w] = incl;
  }
  __syncthreads();
  unsigned long long above = 0;
  bool ok = false;
  if (tid < 256) {
    unsigned long long hi = 0;
    for (int k = w + 1; k < 4; ++k) hi += s_w[k];
    above = above_in + hi + (incl - m);          // mass strictly above bin tid
    ok = c > 0 && above < pq;
    const unsigned long long mk = __ballot(ok), ne = __ballot(c > 0);
    if (lane == 0) {
      s_i[w] = mk ? (__ffsll((long long)mk) - 1) + 64 * w : -1;             // lowest qualifying bin of this wave
      s_i[4 + w] = ne ? (63 - __clzll((long long)ne)) + 64 * w : -1;        // highest non-empty bin of this wave
    }
  }
  __syncthreads();
  int sel = -1;
  for (int k = 0; k < 4 && sel < 0; ++k) sel = s_i[k];
  if (sel < 0) for (int k = 3; k >= 0 && sel < 0; --k) sel = s_i[4 + k];
  if (sel < 0) sel = 0;
  __syncthreads();
  if (tid == sel) s_w[4] = above;
  __syncthreads();
  bin_out = (unsigned)sel; above_out = s_w[4];
  __syncthreads();
}

// order-preserving float -> uint key of the samplers' radix descents (a > b as floats <=> fkey(a) > fkey(b) as unsigned)
__device__ __forceinline__ uint32_t fkey(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// splitmix64: the counter-based RNG shared with oracle/sampling.py
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
