// kernels_sample_mb.hip — multi-block sampler for large vocabularies (V > 32768: the v2 models, 128 256 tokens).
//
// The single-block samplers (kernels_decode.hip) walk the whole vocabulary with ONE CU: 126 logits per thread and
// heavily contended LDS histograms cost 570 us per token on LLaMA-3.1's vocabulary (16 % of the v2 decode step).  Here
// the vocabulary is cut into slices of 8192 (1024 threads x 8 CONSECUTIVE logits, register resident) and the sampler
// becomes a chain of 7 tiny kernels; a kernel boundary inside the captured graph (1.6 us, profiles/r01_launch_probe.txt)
// is the cheapest device-wide hand-off on this part (a software grid barrier costs 6 us, r01_engine_probe.txt):
//   P0  per-slice masked max / first arg-max                                     -> bmax, barg   (+ zero the histograms)
//   P1..P4  radix level 3..0 of the top-p threshold key: per-wave private LDS histograms of (integer mass, count) ->
//           block histogram -> global integer atomics (order independent: exact); every block re-derives the
//           previous level's bin from the global histogram, block 0 publishes it
//   P5  threshold = level-0 bin; kept mass per slice                              -> bkept
//   P6  target = floor(kept * r / 2^32); the slice / thread / element that owns it in index order -> token; advance
//       DecState; gather the token's embedding (first op of the next forward)
// Integer semantics identical to k_sample / k_sample_fast / oracle/sampling.py (q = floor(exp(z - zmax) * 2^31), kept set
// { key >= thr }, inverse-CDF draw in index order with the splitmix64 counter RNG): same tokens, bit for bit.
// TR (SampleArgs::trunc, dtk_set_sampling_ext): min-p and the epsilon cut-off behind top-p.  P5 then leaves every slice's mass of the set
// kept after top-p and min-p (bpre); one more kernel, k_smb_trunc, folds those in slice order into total_m, forms the mass floor
// max(qmin, (int64)((double)eps * (double)total_m)) — above 2^31: the first arg-max alone survives — and leaves the final bkept; P6
// applies the floor.  Without it the chain is the 7 kernels above, unchanged.
// PN (SampleArgs::pen, dtk_set_penalties): the logit transform of sample_inl.h's LogitXf (bias, presence / frequency penalty, DRY, the
// EOS length rules), applied by mb_load — so every kernel of the chain that reloads the row sees the same z' — after the raw values
// have been handed out for the log-sum-exp, before the temperature and the suppression lists.  The block of k_smb_draw that writes the
// token may run before other blocks of its slot have loaded their slice (the hazard draw_snap exists for), so the token is NOT counted
// here: sample_commit leaves it in pen_tok, and k_count_token, a kernel behind the chain, counts it.  The EOS rules need the sequence's
// length, which k_smb_draw's owner block advances: k_smb_max leaves it in SampleMB::cur_snap.  PN = false are the kernels as they were
// before the penalties existed.
// Supports greedy, temperature, top-p and the suppression lists; top-k > 0 stays on the single-block kernel (the API
// re-captures the graph when a sampling configuration needs the other kind).
#include "sample_inl.h"

#define MB_THREADS 1024
#define MB_PER 8
#define MB_SLICE (MB_THREADS * MB_PER)

struct MbElems {
  float z[MB_PER];
  uint32_t key[MB_PER];
  uint32_t q[MB_PER];
};

// the sequence's length for the kernels behind k_smb_max: its snapshot, NOT DecState (k_smb_draw's owner block advances next_pos while
// other blocks of the slot may not have loaded their slice yet)
template <bool PN>
__device__ __forceinline__ int mb_cur(const SampleArgs& a) {
  if constexpr (PN) if (a.len) return a.mb->cur_snap;
  return 0;
}

// this thread's 8 consecutive logits: scaled, suppressed ids -> -inf, keys; out-of-range -> -inf.  raw (k_smb_max<true> only): the
// same loads before the temperature and the suppression lists, out-of-range -> -inf
// PN: z' = LogitXf of every z (bound to the sequence's records and its length `cur`); raw stays raw
template <bool PN = false>
__device__ __forceinline__ void mb_load(const SampleArgs& a, const SamplingDev* sp, bool first, float invT, int base, MbElems& e,
                                        float* raw = nullptr, int cur = 0) {
  const int V = a.V;
  LogitXf xf;
  xf.bind<PN>(a, cur);
  if (base + MB_PER <= V && ((reinterpret_cast<uintptr_t>(a.logits + base) & 15) == 0)) {
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(a.logits + base);
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(a.logits + base + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { e.z[i] = v0[i]; e.z[4 + i] = v1[i]; }
    if (raw) {
#pragma unroll
      for (int i = 0; i < MB_PER; ++i) raw[i] = e.z[i];
    }
    if constexpr (PN) xf.vec<MB_PER>(a, base, e.z);      // (base is a multiple of 8, the tables 16-byte aligned)
#pragma unroll
    for (int i = 0; i < MB_PER; ++i) e.z[i] *= invT;
  } else {
#pragma unroll
    for (int i = 0; i < MB_PER; ++i) {
      const bool in = base + i < V;
      float z = in ? a.logits[base + i] : -INFINITY;
      if (raw) raw[i] = z;
      if constexpr (PN) if (in) z = xf.one(a, base + i, z);
      e.z[i] = in ? z * invT : -INFINITY;
    }
  }
  // suppression lists: which of the (<= 24) ids fall into this thread's 8 elements
  auto ban = [&](int id) {
    const int o = id - base;
#pragma unroll
    for (int i = 0; i < MB_PER; ++i) if (o == i) e.z[i] = -INFINITY;
  };
  for (int j = 0; j < sp->n_bad; ++j) ban(sp->bad_ids[j]);
  for (int j = 0; j < sp->n_always; ++j) ban(sp->always_ids[j]);
  if (first) for (int j = 0; j < sp->n_begin; ++j) ban(sp->begin_ids[j]);
#pragma unroll
  for (int i = 0; i < MB_PER; ++i) e.key[i] = fkey(e.z[i]);
}

__device__ __forceinline__ void mb_mass(MbElems& e, float zmax) {
#pragma unroll
  for (int i = 0; i < MB_PER; ++i) e.q[i] = (uint32_t)(unsigned long long)((double)expf(e.z[i] - zmax) * 2147483648.0);
}

struct MbCommon {
  SamplingDev sp;
  float zmax;
  int argmax;
};

// sampling config -> LDS, global max / first arg-max from the per-slice results of P0
__device__ __forceinline__ void mb_common(const SampleArgs& a, int nblk, MbCommon* cm) {
  const int tid = threadIdx.x;
  if (tid < (int)(sizeof(SamplingDev) / 4)) reinterpret_cast<uint32_t*>(&cm->sp)[tid] = reinterpret_cast<const uint32_t*>(a.sp)[tid];
  if (tid < 64) {   // <= 32 slices: one wave reduces (max, first arg-max)
    float b = tid < nblk ? a.mb->bmax[tid] : -INFINITY; int bi = tid < nblk ? a.mb->barg[tid] : 0x7fffffff;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ob = __shfl_xor(b, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (ob > b || (ob == b && oi < bi)) { b = ob; bi = oi; }
    }
    if (tid == 0) { cm->zmax = b; cm->argmax = bi; }
  }
  __syncthreads();
}

// ---- P0.  LP (SampleArgs::lp_ring): the slice's log-sum-exp state of its raw logits goes out with its maximum
template <bool LP, bool PN>
__global__ __launch_bounds__(MB_THREADS) void k_smb_max(SampleArgs a) {
  if (!sample_bind_slot<PN>(a, blockIdx.y)) return;
  __shared__ SamplingDev s_sp;
  __shared__ float s_f[16];
  __shared__ int s_i[16];
  __shared__ float s_lm[16], s_ls[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, blk = blockIdx.x;
  if (tid < (int)(sizeof(SamplingDev) / 4)) reinterpret_cast<uint32_t*>(&s_sp)[tid] = reinterpret_cast<const uint32_t*>(a.sp)[tid];
  __syncthreads();
  const uint32_t draw = (a.step_override >= 0) ? (uint32_t)a.step_override : a.st->draw;
  const float invT = s_sp.do_sample ? 1.f / s_sp.temperature : 1.f;
  const int cur = sample_cur<PN>(a);       // PN with SampleArgs::len: the sequence's length, for the EOS rules
  MbElems e;
  const int base = blk * MB_SLICE + tid * MB_PER;
  float lm = -INFINITY, ls = 0.f;
  if constexpr (LP) {
    float raw[MB_PER];
    mb_load<PN>(a, &s_sp, draw == 0, invT, base, e, raw, cur);
#pragma unroll
    for (int i = 0; i < MB_PER; ++i) lm = fmaxf(lm, raw[i]);
    if (lm != -INFINITY) {
#pragma unroll
      for (int i = 0; i < MB_PER; ++i) ls += expf(raw[i] - lm);      // out of range: exp(-inf) = 0
    }
    lse_wave(lm, ls);
    if (lane == 0) { s_lm[wave] = lm; s_ls[wave] = ls; }
  } else {
    mb_load<PN>(a, &s_sp, draw == 0, invT, base, e, nullptr, cur);
  }
  float best = -INFINITY; int besti = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < MB_PER; ++i)
    if (base + i < a.V && (e.z[i] > best || (e.z[i] == best && base + i < besti))) { best = e.z[i]; besti = base + i; }
  block_argmax_first<MB_THREADS>(best, besti, s_f, s_i);
  if (tid == 0) {
    a.mb->bmax[blk] = best; a.mb->barg[blk] = besti;
    if constexpr (LP) {      // thread 0 holds wave 0's state: fold the others in wave order
      for (int w = 1; w < 16; ++w) lse_merge(lm, ls, s_lm[w], s_ls[w]);
      a.mb->lmax[blk] = lm; a.mb->lsum[blk] = ls;
    }
    if (blk == 0) { a.mb->draw_snap = draw; a.mb->forced_snap = a.advance ? a.st->force_plus1 : 0; }
    if constexpr (PN) if (a.len && blk == 0) a.mb->cur_snap = cur;
  }
  // the histograms of this step start from zero (P1 is a later kernel)
  if (blk == 0) {
    unsigned long long* hm = &a.mb->hmass[0][0];
    unsigned int* hc = &a.mb->hcnt[0][0];
    for (int i = tid; i < 4 * 256; i += MB_THREADS) { hm[i] = 0ull; hc[i] = 0u; }
  }
}

// bin of radix level `lv` from its global histogram (bin_select_mass, common.h); called by every block, published by block 0
__device__ __forceinline__ void mb_select(const SampleArgs& a, int lv, unsigned long long pq, unsigned long long above_in,
                                          unsigned long long* s_m, unsigned int* s_c, unsigned long long* s_w, int* s_i,
                                          unsigned int& bin_out, unsigned long long& above_out) {
  const int tid = threadIdx.x;
  if (tid < 256) { s_m[tid] = a.mb->hmass[lv][tid]; s_c[tid] = a.mb->hcnt[lv][tid]; }
  __syncthreads();
  bin_select_mass(s_m, s_c, pq, above_in, s_w, s_i, bin_out, above_out);
}

// ---- P1..P4: LV = 3, 2, 1, 0
template <int LV, bool PN>
__global__ __launch_bounds__(MB_THREADS) void k_smb_hist(SampleArgs a, int nblk) {
  if (!sample_bind_slot<PN>(a, blockIdx.y)) return;
  __shared__ MbCommon cm;
  __shared__ unsigned long long w_m[16][256];   // per-wave private histograms: conflicts only inside a wave
  __shared__ unsigned int w_c[16][256];
  __shared__ unsigned long long s_m[256];
  __shared__ unsigned int s_c[256];
  __shared__ unsigned long long s_w[8];
  __shared__ int s_i[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, blk = blockIdx.x;
  mb_common(a, nblk, &cm);
  if (!cm.sp.do_sample || !(cm.sp.top_p < 1.0f)) return;   // greedy / no nucleus: nothing to select (block-uniform)
  const uint32_t draw = (a.step_override >= 0) ? (uint32_t)a.step_override : a.st->draw;
  // selection of the previous level (LV + 1), then this level's prefix
  uint32_t prefix = 0;
  if (LV < 3) {
    // total mass = sum of the level-3 histogram
    unsigned long long total = 0, above = 0;
    if (LV + 1 == 3) {     // total mass = sum of the level-3 bins: the same suffix machinery with pq = 0 (nothing qualifies)
      unsigned long long t = 0;
      if (tid < 256) {
        t = a.mb->hmass[3][tid];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
        if (lane == 0) s_w[wave] = t;
      }
      __syncthreads();
      total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
      __syncthreads();
      if (blk == 0 && tid == 0) a.mb->total = total;
    } else {
      total = a.mb->total; above = a.mb->above[LV + 2];
      for (int l = 3; l > LV + 1; --l) prefix |= a.mb->bin[l] << (l * 8);
    }
    const unsigned long long pq = (unsigned long long)((double)cm.sp.top_p * (double)total);
    unsigned int bin; unsigned long long ab;
    mb_select(a, LV + 1, pq, above, s_m, s_c, s_w, s_i, bin, ab);
    prefix |= bin << ((LV + 1) * 8);
    if (blk == 0 && tid == 0) { a.mb->bin[LV + 1] = bin; a.mb->above[LV + 1] = ab; }
  }
  for (int i = tid; i < 16 * 256; i += MB_THREADS) { (&w_m[0][0])[i] = 0ull; (&w_c[0][0])[i] = 0u; }
  __syncthreads();
  const float invT = 1.f / cm.sp.temperature;
  MbElems e;
  const int base = blk * MB_SLICE + tid * MB_PER;
  mb_load<PN>(a, &cm.sp, draw == 0, invT, base, e, nullptr, mb_cur<PN>(a));
  mb_mass(e, cm.zmax);
  constexpr int shift = LV * 8;
  // run-length aggregation over the thread's 8 consecutive elements (neighbours mostly share the digit), then atomics
  // on the wave's private histogram
  unsigned long long run_q = 0; unsigned int run_c = 0; int run_d = -1;
#pragma unroll
  for (int i = 0; i < MB_PER; ++i) {
    const bool in = base + i < a.V;
    const bool match = in && ((LV == 3) || ((e.key[i] >> (shift + 8)) == (prefix >> (shift + 8))));
    const int d = match ? (int)((e.key[i] >> shift) & 255) : -1;
    if (d != run_d) {
      if (run_d >= 0) { atomicAdd(&w_m[wave][run_d], run_q); atomicAdd(&w_c[wave][run_d], run_c); }
      run_d = d; run_q = 0; run_c = 0;
    }
    if (d >= 0) { run_q += e.q[i]; run_c += 1; }
  }
  if (run_d >= 0) { atomicAdd(&w_m[wave][run_d], run_q); atomicAdd(&w_c[wave][run_d], run_c); }
  __syncthreads();
  if (tid < 256) {
    unsigned long long m = 0; unsigned int c = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) { m += w_m[w][tid]; c += w_c[w][tid]; }
    if (c) { atomicAdd(&a.mb->hmass[LV][tid], m); atomicAdd(&a.mb->hcnt[LV][tid], c); }
  }
  (void)lane;
}

// ---- P5: threshold + kept mass per slice.  TR: the mass of the slice's entries that pass top-p and min-p, to bpre
template <bool TR, bool PN>
__global__ __launch_bounds__(MB_THREADS) void k_smb_kept(SampleArgs a, int nblk) {
  if (!sample_bind_slot<PN>(a, blockIdx.y)) return;
  __shared__ MbCommon cm;
  __shared__ unsigned long long s_m[256];
  __shared__ unsigned int s_c[256];
  __shared__ unsigned long long s_w[8];
  __shared__ int s_i[8];
  __shared__ unsigned long long s_q[16];
  const int tid = threadIdx.x, blk = blockIdx.x;
  mb_common(a, nblk, &cm);
  if (!cm.sp.do_sample) return;
  const uint32_t draw = (a.step_override >= 0) ? (uint32_t)a.step_override : a.st->draw;
  uint32_t thr = 0;
  if (cm.sp.top_p < 1.0f) {
    const unsigned long long total = a.mb->total;
    const unsigned long long pq = (unsigned long long)((double)cm.sp.top_p * (double)total);
    uint32_t prefix = 0;
    for (int l = 3; l > 0; --l) prefix |= a.mb->bin[l] << (l * 8);
    unsigned int bin; unsigned long long ab;
    mb_select(a, 0, pq, a.mb->above[1], s_m, s_c, s_w, s_i, bin, ab);
    thr = prefix | bin;
  }
  if (blk == 0 && tid == 0) a.mb->thr = thr;
  const float invT = 1.f / cm.sp.temperature;
  MbElems e;
  const int base = blk * MB_SLICE + tid * MB_PER;
  mb_load<PN>(a, &cm.sp, draw == 0, invT, base, e, nullptr, mb_cur<PN>(a));
  mb_mass(e, cm.zmax);
  unsigned long long mine = 0;
#pragma unroll
  for (int i = 0; i < MB_PER; ++i)
    if (base + i < a.V && e.key[i] >= thr && (!TR || (long long)e.q[i] >= cm.sp.qmin)) mine += e.q[i];
  const unsigned long long t = block_sum_u64<MB_THREADS>(mine, s_q);
  if (tid == 0) {
    if constexpr (TR) a.mb->bpre[blk] = t; else a.mb->bkept[blk] = t;
  }
}

// ---- TR only, between P5 and P6: the mass floor from the slices' bpre (folded in slice order by every block), the final kept mass per slice
template <bool PN>
__global__ __launch_bounds__(MB_THREADS) void k_smb_trunc(SampleArgs a, int nblk) {
  if (!sample_bind_slot<PN>(a, blockIdx.y)) return;
  __shared__ MbCommon cm;
  __shared__ unsigned long long s_q[16];
  const int tid = threadIdx.x, blk = blockIdx.x;
  mb_common(a, nblk, &cm);
  if (!cm.sp.do_sample) return;
  const uint32_t draw = (a.step_override >= 0) ? (uint32_t)a.step_override : a.st->draw;
  unsigned long long total_m = 0;
  for (int k = 0; k < nblk; ++k) total_m += a.mb->bpre[k];
  uint32_t qfl; bool fb;
  trunc_floor(cm.sp.qmin, cm.sp.eps, total_m, qfl, fb);
  if (blk == 0 && tid == 0) { a.mb->qfl = qfl; a.mb->fb = fb ? 1 : 0; }
  const uint32_t thr = a.mb->thr;
  const float invT = 1.f / cm.sp.temperature;
  MbElems e;
  const int base = blk * MB_SLICE + tid * MB_PER;
  mb_load<PN>(a, &cm.sp, draw == 0, invT, base, e, nullptr, mb_cur<PN>(a));
  mb_mass(e, cm.zmax);
  unsigned long long mine = 0;
#pragma unroll
  for (int i = 0; i < MB_PER; ++i)
    if (base + i < a.V && sample_kept<true>(e.key[i], e.q[i], base + i, thr, qfl, fb, cm.argmax)) mine += e.q[i];
  const unsigned long long t = block_sum_u64<MB_THREADS>(mine, s_q);
  if (tid == 0) a.mb->bkept[blk] = t;
}

// ---- P6: draw (or arg-max), token ring, DecState, embedding gather.  LP: thread 0 of the block that writes the token folds the
// slices' log-sum-exp states in slice order and stores the token's (logprob, sample_logprob)
template <bool LP, bool TR, bool PN>
__global__ __launch_bounds__(MB_THREADS) void k_smb_draw(SampleArgs a, int nblk) {
  if (!sample_bind_slot<PN>(a, blockIdx.y)) return;
  __shared__ MbCommon cm;
  __shared__ unsigned long long scan[MB_THREADS];
  __shared__ int s_token;
  __shared__ unsigned int s_tokq;          // LP: the chosen token's integer mass, published by the thread that chose it
  const int tid = threadIdx.x, blk = blockIdx.x;
  mb_common(a, nblk, &cm);
  // the snapshot of k_smb_max, NOT DecState: the block that owns the token advances DecState (draw, force_plus1) at its end,
  // and with more blocks than the chip holds at once (v2-8b: 16 slices x 64 slots) a block of the same slot can start after
  // that — it would see the next step's draw index / a cleared force flag, pick an owner of its own and advance a second time
  const uint32_t draw = a.mb->draw_snap;
  const int forced = a.mb->forced_snap;
  const bool sampling = cm.sp.do_sample != 0;
  if (tid == 0) s_token = -1;
  __syncthreads();
  unsigned long long kept = 0;
  bool owner = false;
  if (!sampling) {
    owner = blk == 0;
    if (owner && tid == 0) s_token = cm.argmax;
    if (a.probs_out) {
      const int base = blk * MB_SLICE + tid * MB_PER;
      for (int i = 0; i < MB_PER; ++i) if (base + i < a.V) a.probs_out[base + i] = (base + i == cm.argmax) ? 1.f : 0.f;
    }
  } else {
    unsigned long long before = 0;
    for (int k = 0; k < nblk; ++k) { const unsigned long long v = a.mb->bkept[k]; if (k < blk) before += v; kept += v; }
    const unsigned long long target = draw_target(cm.sp.seed, draw, kept);
    const unsigned long long mine_blk = a.mb->bkept[blk];
    owner = mine_blk > 0 && target >= before && target < before + mine_blk;     // exactly one slice
    if (owner || a.probs_out) {
      const uint32_t thr = a.mb->thr;
      const float invT = 1.f / cm.sp.temperature;
      MbElems e;
      const int base = blk * MB_SLICE + tid * MB_PER;
      mb_load<PN>(a, &cm.sp, draw == 0, invT, base, e, nullptr, mb_cur<PN>(a));
      mb_mass(e, cm.zmax);
      uint32_t qfl = 0; bool fb = false;
      if constexpr (TR) { qfl = a.mb->qfl; fb = a.mb->fb != 0; }
      auto kept_el = [&](int i) -> bool { return sample_kept<TR>(e.key[i], e.q[i], base + i, thr, qfl, fb, cm.argmax); };
      if (a.probs_out)
        for (int i = 0; i < MB_PER; ++i)
          if (base + i < a.V) a.probs_out[base + i] = kept_el(i) ? (float)((double)e.q[i] / (double)kept) : 0.f;
      if (owner) {
        unsigned long long mine = 0;
#pragma unroll
        for (int i = 0; i < MB_PER; ++i) if (base + i < a.V && kept_el(i)) mine += e.q[i];
        block_scan_u64<MB_THREADS>(scan, mine);      // block-uniform branch (owner): barriers are safe
        const unsigned long long excl = before + scan[tid] - mine;
        if (mine > 0 && target >= excl && target < excl + mine) {
          unsigned long long run = excl;
#pragma unroll
          for (int i = 0; i < MB_PER; ++i) {
            if (base + i < a.V && kept_el(i)) {
              if (target < run + e.q[i] && s_token < 0) { s_token = base + i; if constexpr (LP) s_tokq = e.q[i]; }
              run += e.q[i];
            }
          }
        }
      }
    }
  }
  __syncthreads();
  if (forced > 0) owner = blk == 0;     // nothing was asked of the (stale) logits: exactly one block writes the token
  if (!owner) return;
  float2 lp = make_float2(0.f, 0.f); float lse = 0.f;
  if constexpr (LP) if (tid == 0 && forced <= 0) {      // the slices' log-sum-exp states, folded in slice order
    float lm = a.mb->lmax[0], ls = a.mb->lsum[0];
    for (int k = 1; k < nblk; ++k) lse_merge(lm, ls, a.mb->lmax[k], a.mb->lsum[k]);
    lp = lp_pair(a.logits[s_token], lm, ls, sampling, sampling ? s_tokq : 0u, kept);
    lse = lm + logf(ls);
  }
  sample_commit<LP, PN, MB_THREADS>(a, s_token, forced, draw, lp, lse);
}

template <bool PN>
static void launch_sample_mb_t(const SampleArgs& a, hipStream_t s) {
  const int nblk = (a.V + MB_SLICE - 1) / MB_SLICE;   // <= DTK_SAMPLE_MB_MAX_SLICES
  const dim3 g(nblk, a.bs ? a.nslots : 1), b(MB_THREADS);
  dispatch_lp_tr(a, [&](auto lp, auto tr) {
    constexpr bool LP = decltype(lp)::value, TR = decltype(tr)::value;
    hipLaunchKernelGGL((k_smb_max<LP, PN>), g, b, 0, s, a);
    hipLaunchKernelGGL((k_smb_hist<3, PN>), g, b, 0, s, a, nblk);
    hipLaunchKernelGGL((k_smb_hist<2, PN>), g, b, 0, s, a, nblk);
    hipLaunchKernelGGL((k_smb_hist<1, PN>), g, b, 0, s, a, nblk);
    hipLaunchKernelGGL((k_smb_hist<0, PN>), g, b, 0, s, a, nblk);
    hipLaunchKernelGGL((k_smb_kept<TR, PN>), g, b, 0, s, a, nblk);
    if constexpr (TR) hipLaunchKernelGGL(k_smb_trunc<PN>, g, b, 0, s, a, nblk);
    hipLaunchKernelGGL((k_smb_draw<LP, TR, PN>), g, b, 0, s, a, nblk);
  });
}
// a.pen == nullptr (no sequence of this launch has a presence / frequency penalty): the PN = false instantiations, the chain as it was
void launch_sample_mb(const SampleArgs& a, hipStream_t s) {
  if (a.pen) launch_sample_mb_t<true>(a, s); else launch_sample_mb_t<false>(a, s);
}
