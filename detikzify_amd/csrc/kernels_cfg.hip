// kernels_cfg.hip — classifier-free guidance of the batched decode step (dtk_set_guidance).
//
// A guided pair is two batch slots: the conditional slot c and the unconditional slot u.  In front of everything the step does with
// the pending raw logits (k_top_logits, the sampler chain), the conditional row is replaced in place by
//     out[v] = g * ((zc[v] - Lc) - (zu[v] - Lu)) + (zu[v] - Lu),   Lc = logsumexp(zc), Lu = logsumexp(zu)
// in fp32, every operation rounded on its own (no fma): HF's UnbatchedClassifierFreeGuidanceLogitsProcessor.  Behind the sampler
// k_cfg_follow hands the token the conditional slot's chain chose to the unconditional slot, which forwards it too.
//
// Two launches, grid (slice, pair), no atomics and no waits between blocks:
//   k_cfg_lse  block (s, p) walks elements [s * per, (s + 1) * per) of both rows and stores one online log-sum-exp state (max, sum
//              exp(z - max)) per (pair, row, slice).
//   k_cfg_mix  block (s, p) folds the slices' states of both rows — the maximum first (exact in any order), then the rescaled sums
//              added in slice order — into Lc and Lu and writes out for its slice over the conditional row.
// The launch shape is a function of V alone (cfg_shape): 256 threads, a thread owns 4 consecutive elements per 1024-element stride,
// per = 1024 * ceil(V / (1024 * 128)) elements per slice, so at most DTK_CFG_MAX_SLICES = 128 slices (126 at V = 128 256: a block per
// 4 KiB of each row, one 16-byte load per thread and row — the rows are 0.5 MB, the kernels are latency- not bandwidth-bound, and a
// block per pair would walk them with one CU).  Which element a thread pushes when, and how the states are folded, depends on
// nothing else — not on the slot indices, not on the other pairs, not on where a row starts in memory — so the bits repeat.
// A row starts at slot * V floats: with V % 4 != 0 it is not 16-byte aligned for every slot.  A thread's 4 elements are then read (and
// written) with scalar accesses, as is the ragged group at the end of the row; the element-to-thread map stays the same.
#include "kernels.h"

#define CFG_THREADS 256
#define CFG_STRIDE (CFG_THREADS * 4)      // elements one pass of the block covers

void cfg_shape(int V, int* per_out, int* nslices_out) {
  const int k = (V + CFG_STRIDE * DTK_CFG_MAX_SLICES - 1) / (CFG_STRIDE * DTK_CFG_MAX_SLICES);
  const int per = CFG_STRIDE * (k < 1 ? 1 : k);
  *per_out = per;
  *nslices_out = (V + per - 1) / per;
}

namespace {

// the 4 elements [i, i + 4) of a row of V; vec: the row is 16-byte aligned (block-uniform).  Elements >= V are not touched.
__device__ __forceinline__ int cfg_load4(const float* row, int i, int V, bool vec, float* z) {
  if (vec && i + 4 <= V) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + i);
    z[0] = v[0]; z[1] = v[1]; z[2] = v[2]; z[3] = v[3];
    return 4;
  }
  int n = 0;
  for (; n < 4 && i + n < V; ++n) z[n] = row[i + n];
  return n;
}

// out of one element: four fp32 operations, four roundings (what __fsub_rn / __fmul_rn / __fadd_rn promise).  Written with plain
// operators and contraction switched off for this body, as decay_apply: the _rn intrinsics are inline functions of the HIP headers whose
// operators carry the build's contract flag, so a product and a sum made of them are fused into one fma after inlining (measured: one
// ulp off the replay at g = 1.5)
__device__ __forceinline__ float cfg_out(float zc, float zu, float Lc, float Lu, float g) {
#pragma clang fp contract(off)
  const float lc = zc - Lc;
  const float lu = zu - Lu;
  const float d = lc - lu;
  const float p = g * d;
  return p + lu;
}

// the slice's state of one row, in thread 0 (every thread of the block calls it)
__device__ __forceinline__ float2 cfg_row_state(const float* row, int i0, int i1, int V, float* s_m, float* s_s) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  float m = -INFINITY, s = 0.f;
  for (int i = i0 + tid * 4; i < i1; i += CFG_STRIDE) {
    float z[4];
    const int n = cfg_load4(row, i, V, vec, z);
    for (int e = 0; e < n; ++e) lse_push(m, s, z[e]);
  }
  lse_wave(m, s);
  if (lane == 0) { s_m[wave] = m; s_s[wave] = s; }
  __syncthreads();
  float2 r = make_float2(-INFINITY, 0.f);
  if (tid == 0) {
    r.x = s_m[0]; r.y = s_s[0];
    for (int w = 1; w < CFG_THREADS / 64; ++w) lse_merge(r.x, r.y, s_m[w], s_s[w]);
  }
  __syncthreads();
  return r;
}

// Block-uniform: the entry is unused (cond < 0: a reserved table position without a pair — nothing else of the step is read), its
// conditional slot sits this step out, or the pair forwards forced tokens this step (dtk_resume_slot; dtk_decode_batch_launch lets a pair
// through only with both slots in that phase or neither).  The forced step reads no logits: the rows are those of the slots' earlier
// sequences, or were never written, so nothing is folded or mixed — the sampler forwards each slot's own token whatever the rows hold
__device__ __forceinline__ bool cfg_pair_idle(const CfgArgs& a, const CfgPair& p) {
  if (p.cond < 0) return true;
  if (a.bs && !a.bs->active[p.cond]) return true;
  return a.st && a.st[p.cond].force_plus1 != 0;
}

__global__ __launch_bounds__(CFG_THREADS) void k_cfg_lse(CfgArgs a) {
  const CfgPair p = a.pairs[blockIdx.y];
  if (a.forced && p.cond >= 0 && blockIdx.x == 0 && threadIdx.x == 0 && (!a.bs || a.bs->active[p.cond]))
    a.forced[blockIdx.y] = a.st[p.cond].force_plus1 != 0;
  if (cfg_pair_idle(a, p)) return;
  __shared__ float s_m[CFG_THREADS / 64], s_s[CFG_THREADS / 64];
  const int i0 = blockIdx.x * a.per, i1 = min(a.V, i0 + a.per);
  float2* part = a.part + (size_t)blockIdx.y * 2 * DTK_CFG_MAX_SLICES;
  const float2 c = cfg_row_state(a.logits + (size_t)p.cond * a.stride, i0, i1, a.V, s_m, s_s);
  const float2 u = cfg_row_state(a.logits + (size_t)p.uncond * a.stride, i0, i1, a.V, s_m, s_s);
  if (threadIdx.x == 0) { part[blockIdx.x] = c; part[DTK_CFG_MAX_SLICES + blockIdx.x] = u; }
}

__global__ __launch_bounds__(CFG_THREADS) void k_cfg_mix(CfgArgs a) {
  const CfgPair p = a.pairs[blockIdx.y];
  if (cfg_pair_idle(a, p)) return;      // (the sampler, which clears force_plus1, runs behind this kernel)
  __shared__ float s_t[2][DTK_CFG_MAX_SLICES];
  __shared__ float s_max[2][2];
  __shared__ float s_L[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nsl = gridDim.x;
  // threads [0, 128) take the conditional row's slices, [128, 256) the unconditional row's: one state per thread
  const int r = tid >> 7, sl = tid & (DTK_CFG_MAX_SLICES - 1);
  const float2 st = sl < nsl ? a.part[((size_t)blockIdx.y * 2 + r) * DTK_CFG_MAX_SLICES + sl] : make_float2(-INFINITY, 0.f);
  const float wm = wave_max(st.x);
  if (lane == 0) s_max[r][wave & 1] = wm;
  __syncthreads();
  const float M = fmaxf(s_max[r][0], s_max[r][1]);      // finite: every slice holds at least one finite logit
  s_t[r][sl] = sl < nsl ? __fmul_rn(st.y, expf(st.x - M)) : 0.f;
  __syncthreads();
  if (sl == 0) {
    float S = 0.f;
    for (int i = 0; i < nsl; ++i) S = __fadd_rn(S, s_t[r][i]);      // slice order
    s_L[r] = M + logf(S);
  }
  __syncthreads();
  const float Lc = s_L[0], Lu = s_L[1], g = p.scale;
  if (tid == 0 && blockIdx.x == 0) a.lse[blockIdx.y] = make_float2(Lc, Lu);
  float* zc = a.logits + (size_t)p.cond * a.stride;
  const float* zu = a.logits + (size_t)p.uncond * a.stride;
  const bool vc = (reinterpret_cast<uintptr_t>(zc) & 15) == 0, vu = (reinterpret_cast<uintptr_t>(zu) & 15) == 0;
  const int i0 = blockIdx.x * a.per, i1 = min(a.V, i0 + a.per);
  for (int i = i0 + tid * 4; i < i1; i += CFG_STRIDE) {
    float c[4], u[4], o[4];
    const int n = cfg_load4(zc, i, a.V, vc, c);
    cfg_load4(zu, i, a.V, vu, u);
    for (int e = 0; e < n; ++e) o[e] = cfg_out(c[e], u[e], Lc, Lu, g);
    if (vc && n == 4) { f32x4 v; v[0] = o[0]; v[1] = o[1]; v[2] = o[2]; v[3] = o[3]; *reinterpret_cast<f32x4*>(zc + i) = v; }
    else for (int e = 0; e < n; ++e) zc[i + e] = o[e];
  }
}

// behind the sampler (and k_count_token): the unconditional slot of every active pair takes over what the conditional slot's chain
// left — DecState::token, the gathered embedding row, the token ring entry and the lp / lse / top ring entries of the step.  The
// unconditional slot's own sampler block has advanced that slot's position already.  On the forced step of a resumed pair both samplers
// have forwarded their slot's own last prompt token (token, embedding row, token ring, NaN log-probabilities): nothing is handed over
__global__ __launch_bounds__(CFG_THREADS) void k_cfg_follow(CfgFollowArgs a) {
  const CfgPair p = a.pairs[blockIdx.x];
  if (p.cond < 0 || !a.bs->active[p.cond] || (a.forced && a.forced[blockIdx.x])) return;
  const int tid = threadIdx.x;
  const size_t ri = (size_t)((unsigned)a.bs->step % (unsigned)a.ring) * DTK_MAX_BATCH;
  if (tid == 0) {
    a.st[p.uncond].token = a.st[p.cond].token;
    a.tok_ring[ri + p.uncond] = a.tok_ring[ri + p.cond];
    if (a.lp_ring) a.lp_ring[ri + p.uncond] = a.lp_ring[ri + p.cond];
    if (a.lse_ring) a.lse_ring[ri + p.uncond] = a.lse_ring[ri + p.cond];
  }
  if (a.top_ring && tid >= 64 && tid < 64 + DTK_MAX_TOP) {
    const int j = tid - 64;
    a.top_ring[ri + p.uncond].id[j] = a.top_ring[ri + p.cond].id[j];
    a.top_ring[ri + p.uncond].z[j] = a.top_ring[ri + p.cond].z[j];
  }
  const u32x4* src = reinterpret_cast<const u32x4*>(a.x + (size_t)p.cond * a.d);
  u32x4* dst = reinterpret_cast<u32x4*>(a.x + (size_t)p.uncond * a.d);
  for (int c = tid; c < (a.d >> 3); c += CFG_THREADS) dst[c] = src[c];
}

}  // namespace

void launch_cfg_mix(const CfgArgs& a, hipStream_t s) {
  if (a.n_pairs <= 0) return;
  CfgArgs b = a;
  int nsl = 0;
  cfg_shape(a.V, &b.per, &nsl);
  const dim3 g(nsl, a.n_pairs), t(CFG_THREADS);
  hipLaunchKernelGGL(k_cfg_lse, g, t, 0, s, b);
  hipLaunchKernelGGL(k_cfg_mix, g, t, 0, s, b);
}
void launch_cfg_follow(const CfgFollowArgs& a, hipStream_t s) {
  if (a.n_pairs <= 0) return;
  hipLaunchKernelGGL(k_cfg_follow, dim3(a.n_pairs), dim3(CFG_THREADS), 0, s, a);
}
