// sample_inl.h — what the three sampler families share (device-only inlines): k_sample and k_sample_fast (kernels_decode.hip) and the
// k_smb_* chain (kernels_sample_mb.hip).  One definition each of the batched slot view, the logit transform of the PN instantiations,
// the block reductions, the integer rules of the draw and the commit.  A new logits processor goes into LogitXf (both forms); a new
// value stored with the token goes into sample_commit.  DESIGN.md §3.1n.
#pragma once
#include "kernels.h"

// ---- the batched slot view: block (or grid row) `slot` works on that slot's buffers; false = the slot is not part of this step.
// Single sequence (a.bs null): the arguments as they are.  The rings are indexed by the step here, so a.ring becomes 1 behind it
template <bool PN>
__device__ __forceinline__ bool sample_bind_slot(SampleArgs& a, int slot) {
  if (!a.bs) return true;
  if (!a.bs->active[slot]) return false;
  const size_t ri = (size_t)((unsigned)a.bs->step % (unsigned)a.ring) * DTK_MAX_BATCH + slot;
  a.logits += (size_t)slot * a.logits_stride;
  a.sp += slot;
  a.st += slot;
  a.x += (size_t)slot * a.d;
  a.tok_ring += ri;
  if (a.lp_ring) a.lp_ring += ri;      // (the launchers pick LP from a.lp_ring)
  if (a.lse_ring) a.lse_ring += ri;
  if (a.mb) a.mb += slot;
  if constexpr (PN) {
    a.pen += slot; a.pen_cnt += (size_t)slot * a.pen_stride; a.pen_tok += slot;
    if (a.dry) { a.dry += slot; a.dry_m += (size_t)slot * a.dry_stride; }
    if (a.len) { a.len += slot; a.len_m += (size_t)slot * a.len_m_stride; a.bias += (size_t)slot * a.bias_stride; }
  }
  a.ring = 1;
  a.step_override = -1;
  return true;
}

// the sequence's length for the EOS rules, read where DecState is still this step's (k_sample, k_sample_fast, k_smb_max)
template <bool PN>
__device__ __forceinline__ int sample_cur(const SampleArgs& a) {
  if constexpr (PN) if (a.len) return a.len_cur >= 0 ? a.len_cur : a.st->next_pos;
  return 0;
}

// ---- the logit transform of the PN instantiations: raw -> z' = eos(dry(pen(bias(raw)))), in that order, in front of the temperature and
// the suppression lists (which stay with the callers: their shape differs per family).  Bound once per block from the sequence's records;
// pn, dr, sh.bias and sh.ne are block-uniform, and a sequence without the value reads nothing of its table.  Where the table holds 0
// for an id the logit keeps its bits, so the packed form's zero-word tests skip what would change nothing.
struct LogitXf {
  float pp = 0.f, fp = 0.f; bool pn = false;       // SampleArgs::pen: the sequence's two values; pn = it has some
  const float* dpen = nullptr; bool dr = false;    // SampleArgs::dry: the sequence's pen[M]; dr = it has a multiplier
  ShapeRt sh;                                      // SampleArgs::len: the bias table and the EOS rule of length `cur`

  template <bool PN>
  __device__ __forceinline__ void bind(const SampleArgs& a, int cur) {
    if constexpr (PN) {
      pp = a.pen->pp; fp = a.pen->fp; pn = pp != 0.f || fp != 0.f;
      if (a.dry) { dr = a.dry->on != 0; dpen = a.dry->pen; }
      if (a.len) sh = shape_bind(a.len, a.len_m, a.bias, cur);
    }
  }
  // id i, whose raw logit the caller has loaded
  __device__ __forceinline__ float one(const SampleArgs& a, int i, float z) const {
    if (sh.bias) z = bias_apply(z, sh.bias[i]);
    if (pn) z = pen_apply(z, a.pen_cnt[i], pp, fp);
    if (dr) z = dry_apply(z, a.dry_m[i], dpen);
    if (sh.ne) z = eos_apply(z, i, sh);
    return z;
  }
  // ids [base, base + N), base a multiple of N, N = 4 or 8; v (f32x4 or float[N]) holds their raw logits.  Per 4 ids the biases are one
  // 16-byte load, the counts one 8-byte word, the match lengths one 4-byte word
  template <int N, class Vec>
  __device__ __forceinline__ void vec(const SampleArgs& a, int base, Vec& v) const {
    static_assert(N == 4 || N == 8, "4 or 8 consecutive ids");
#pragma unroll
    for (int g = 0; g < N / 4; ++g) {
      const int i = base + 4 * g;
      if (sh.bias) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(sh.bias + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * g + e] = bias_apply(v[4 * g + e], b[e]);
      }
      if (pn) {
        const uint2 cw = *reinterpret_cast<const uint2*>(a.pen_cnt + i);
        if ((cw.x | cw.y) != 0u) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[4 * g + e] = pen_apply(v[4 * g + e], ((e < 2 ? cw.x : cw.y) >> ((e & 1) * 16)) & 0xffffu, pp, fp);
        }
      }
      if (dr) {
        const uint32_t mw = *reinterpret_cast<const uint32_t*>(a.dry_m + i);
        if (mw != 0u) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[4 * g + e] = dry_apply(v[4 * g + e], (mw >> (8 * e)) & 0xffu, dpen);
        }
      }
      for (int j = 0; j < sh.ne; ++j) {      // at most 8 EOS ids, and only at a length where a rule applies
        const int o = sh.eos[j] - i;
        if (o < 0 || o >= 4) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) if (e == o) v[4 * g + e] = eos_apply(v[4 * g + e], i + e, sh);
      }
    }
  }
};

// ---- block reductions over caller-provided LDS (one entry per wave).  Every thread of the block calls them: they contain barriers
// (max, FIRST arg-max): the result is thread 0's.  Anything else the caller's lanes 0 left in LDS before the call is visible behind it
template <int THREADS>
__device__ __forceinline__ void block_argmax_first(float& best, int& besti, float* s_f, int* s_i) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(besti, off, 64);
    if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
  }
  if ((tid & 63) == 0) { s_f[tid >> 6] = best; s_i[tid >> 6] = besti; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < THREADS / 64; ++w)
      if (s_f[w] > best || (s_f[w] == best && s_i[w] < besti)) { best = s_f[w]; besti = s_i[w]; }
  }
}
// the block's total of v: the return value of thread 0 (integers: exact in any order)
template <int THREADS>
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* s_q) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((tid & 63) == 0) s_q[tid >> 6] = v;
  __syncthreads();
  unsigned long long t = 0;
  if (tid == 0) for (int w = 0; w < THREADS / 64; ++w) t += s_q[w];
  return t;
}
// inclusive scan in thread order (Hillis-Steele): scan[t] = mine(0) + ... + mine(t)
template <int THREADS>
__device__ __forceinline__ void block_scan_u64(unsigned long long* scan, unsigned long long mine) {
  const int tid = threadIdx.x;
  scan[tid] = mine;
  __syncthreads();
  for (int off = 1; off < THREADS; off <<= 1) {
    unsigned long long v = 0;
    if (tid >= off) v = scan[tid - off];
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
}

// ---- the integer rules shared with oracle/sampling.py
// the draw's target in [0, kept): floor(kept * r / 2^32), r the 32 high bits of the counter RNG at this draw
__device__ __forceinline__ unsigned long long draw_target(uint64_t seed, uint32_t draw, unsigned long long kept) {
  const uint64_t r = splitmix64(seed ^ (0xD1B54A32D192ED03ull * (uint64_t)(draw + 1))) >> 32;
  return __umul64hi(kept, r << 32);
}
// TR: the mass floor of min-p and epsilon, max(qmin, (int64)((double)eps * (double)total_m)), total_m the mass kept behind top-p and
// min-p.  A floor above 2^31 leaves nothing: fb, the first arg-max alone survives
__device__ __forceinline__ void trunc_floor(int64_t qmin, float eps, unsigned long long total_m, uint32_t& qfl, bool& fb) {
  unsigned long long fl = (unsigned long long)qmin;
  const unsigned long long qe = (unsigned long long)((double)eps * (double)total_m);
  if (qe > fl) fl = qe;
  fb = fl > 2147483648ull;
  qfl = fb ? 0u : (uint32_t)fl;
}
// id `id` (key, integer mass q) is in the final set
template <bool TR>
__device__ __forceinline__ bool sample_kept(uint32_t key, uint32_t q, int id, uint32_t thr, uint32_t qfl, bool fb, int amax) {
  if constexpr (TR) return fb ? (id == amax) : (key >= thr && q >= qfl);
  else return key >= thr;
}

// ---- the commit, by the one block that owns the token: thread 0 writes the token ring and (LP) the token's (logprob, sample_logprob)
// and logsumexp — NaN for a forced token, which was not sampled —, advances DecState and leaves the token for k_count_token (PN); every
// thread gathers the token's embedding row into the residual stream (first op of the forward that follows).  (lp, lse) are thread 0's.
// A resumed slot (dtk_resume_slot) forwards the last token of its prompt (forced = token + 1) instead of the sampled one: the draw
// counter, and with it the begin-suppress rule of the first SAMPLED token, does not move
template <bool LP, bool PN, int THREADS>
__device__ __forceinline__ void sample_commit(const SampleArgs& a, int tok_sampled, int forced, uint32_t draw, float2 lp, float lse) {
  const int tid = threadIdx.x;
  const int tok = forced > 0 ? forced - 1 : tok_sampled;
  if (tid == 0) {
    const uint32_t ri = a.bs ? 0u : draw % (uint32_t)a.ring;      // (batched: sample_bind_slot applied the ring index)
    a.tok_ring[ri] = (int64_t)tok;
    if constexpr (LP) {
      a.lp_ring[ri] = forced > 0 ? make_float2(__builtin_nanf(""), __builtin_nanf("")) : lp;
      if (a.lse_ring) a.lse_ring[ri] = forced > 0 ? __builtin_nanf("") : lse;
    }
    if (a.advance) {
      a.st->token = tok;
      a.st->pos = a.st->next_pos;
      a.st->next_pos = a.st->next_pos + 1;
      a.st->draw = forced > 0 ? draw : draw + 1;
      if (forced > 0) a.st->force_plus1 = 0;
      if constexpr (PN) *a.pen_tok = forced > 0 ? -1 : tok;      // a forced token is among the ids the table was built from
    }
  }
  if (a.advance) {
    const u32x4* src = reinterpret_cast<const u32x4*>(a.embed + (size_t)tok * a.d);
    u32x4* dst = reinterpret_cast<u32x4*>(a.x);
    for (int c = tid; c < (a.d >> 3); c += THREADS) dst[c] = src[c];
  }
}
