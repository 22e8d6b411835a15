// kernels_top.hip — the slice-parallel selection of dtk_set_option "top_logprobs" (DESIGN §3.1f): the TopRec k_top_logits
// (kernels_decode.hip) writes, bit for bit, in two launches.
//
// k_top_logits is one block per sequence that walks the whole row k times: right at V = 32 256, the wrong shape at V = 128 256, where
// one CU reads 513 KB eight times over.  Here the row is cut into slices of L <= 8192 logits, as the multi-block sampler cuts it:
//   k_top_slice  grid (slices, rows), 256 threads.  A block loads its slice ONCE, 32 values per thread in registers, and extracts the
//                slice's k first entries in k rounds from the registers: a thread-local best strictly behind the previous pick, a
//                butterfly per wave, the four waves' picks through LDS.  The k (z, id) candidates go to scratch[row][slice]; a slice
//                with fewer than k entries pads with (-inf, 0x7fffffff), which top_before puts behind every real entry, a real -inf
//                logit included (its id is smaller).
//   k_top_merge  one block of 256 threads per row, one candidate per thread: the k first of the <= 32 x 8 candidates, in k rounds
//                of the same shape, written to the ring entry k_top_logits would have written.
// The order (z descending, id ascending) is total on real entries and every entry of the row's first k is among its slice's first
// k, so the result is k_top_logits' whatever L is.  No atomics, no hand-off between blocks of a launch and no assumption about which
// blocks are resident together: the kernel boundary is the dependency.  Both kernels read DecState / BatchState in front of the
// sampler, as k_top_logits does: an inactive slot writes nothing, a forced token gets (-1, NaN) in its first k entries.
#include "kernels.h"

#define TOPS_THREADS 256
#define TOPS_PER (DTK_TOP_MAX_L / TOPS_THREADS)      // 32 values per thread

namespace {

// the block's best of (bz, bi) under top_before, in every thread; s_z / s_i: one entry per wave.  Two barriers: the second one frees
// the LDS entries for the next round
__device__ __forceinline__ void top_block_best(float& bz, int& bi, float* s_z, int* s_i) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float oz = __shfl_xor(bz, off, 64); const int oi = __shfl_xor(bi, off, 64);
    if (top_before(oz, oi, bz, bi)) { bz = oz; bi = oi; }
  }
  if (lane == 0) { s_z[wave] = bz; s_i[wave] = bi; }
  __syncthreads();
  bz = s_z[0]; bi = s_i[0];
#pragma unroll
  for (int w = 1; w < TOPS_THREADS / 64; ++w)
    if (top_before(s_z[w], s_i[w], bz, bi)) { bz = s_z[w]; bi = s_i[w]; }
  __syncthreads();
}

__global__ __launch_bounds__(TOPS_THREADS) void k_top_slice(TopArgs a) {
  const int row = blockIdx.y, slice = blockIdx.x, tid = threadIdx.x;
  const float* z = a.logits;
  const DecState* st = a.st;
  if (a.bs) {
    if (!a.bs->active[row]) return;
    z += (size_t)row * a.logits_stride;
    st += row;
  }
  if (st->force_plus1 > 0) return;       // k_top_merge writes the forced token's record; it reads no candidate
  const int lo = slice * a.L;
  const int n = min(a.L, a.V - lo);      // 1 .. L entries (the grid has ceil(V / L) slices)
  // (an entry outside the slice is -inf and never a candidate: the rounds test the index, not the value)
  float v[TOPS_PER];
#pragma unroll
  for (int j = 0; j < TOPS_PER; ++j) {
    const int i = j * TOPS_THREADS + tid;
    v[j] = i < n ? z[lo + i] : -INFINITY;
  }
  __shared__ float s_z[TOPS_THREADS / 64];
  __shared__ int s_i[TOPS_THREADS / 64];
  TopRec* cand = a.scratch + (size_t)row * DTK_TOP_MAX_SLICES + slice;
  float lz = INFINITY; int lid = -1;
  for (int r = 0; r < a.k; ++r) {
    float bz = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < TOPS_PER; ++j) {
      const int i = j * TOPS_THREADS + tid;
      if (i < n && top_before(lz, lid, v[j], lo + i) && top_before(v[j], lo + i, bz, bi)) { bz = v[j]; bi = lo + i; }
    }
    top_block_best(bz, bi, s_z, s_i);
    lz = bz; lid = bi;                   // (the padding entry once the slice is exhausted: nothing is strictly behind it)
    if (tid == 0) { cand->id[r] = bi; cand->z[r] = bz; }
  }
}

__global__ __launch_bounds__(TOPS_THREADS) void k_top_merge(TopArgs a) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const DecState* st = a.st;
  TopRec* out;
  if (a.bs) {
    if (!a.bs->active[row]) return;
    st += row;
    out = a.top_ring + (size_t)((unsigned)a.bs->step % (unsigned)a.ring) * DTK_MAX_BATCH + row;
  } else out = a.top_ring + st->draw % (uint32_t)a.ring;
  if (st->force_plus1 > 0) {             // a forced token was not sampled from these (stale) logits
    if (tid < a.k) { out->id[tid] = -1; out->z[tid] = __builtin_nanf(""); }
    return;
  }
  // candidate tid = entry tid % 8 of slice tid / 8; beyond the row's slices, and beyond k within a slice: the padding entry
  const int nslices = (a.V + a.L - 1) / a.L;
  const int s = tid / DTK_MAX_TOP, e = tid % DTK_MAX_TOP;
  float cz = -INFINITY; int ci = 0x7fffffff;
  if (s < nslices && e < a.k) {
    const TopRec* cand = a.scratch + (size_t)row * DTK_TOP_MAX_SLICES + s;
    cz = cand->z[e]; ci = cand->id[e];
  }
  __shared__ float s_z[TOPS_THREADS / 64];
  __shared__ int s_i[TOPS_THREADS / 64];
  float lz = INFINITY; int lid = -1;
  for (int r = 0; r < a.k; ++r) {
    float bz = -INFINITY; int bi = 0x7fffffff;
    if (top_before(lz, lid, cz, ci)) { bz = cz; bi = ci; }
    top_block_best(bz, bi, s_z, s_i);
    lz = bz; lid = bi;
    if (tid == 0) { out->id[r] = bi; out->z[r] = bz; }
  }
}

}  // namespace

static_assert(DTK_TOP_MAX_SLICES * DTK_MAX_TOP == TOPS_THREADS, "k_top_merge holds one candidate per thread");
static_assert(TOPS_PER * TOPS_THREADS == DTK_TOP_MAX_L, "k_top_slice holds a whole slice in registers");

bool top_sliced_ok(int V, int L) {
  return V >= 1 && L >= 1 && L <= DTK_TOP_MAX_L && ((size_t)V + L - 1) / L <= (size_t)DTK_TOP_MAX_SLICES;
}

void launch_top_sliced(const TopArgs& a, hipStream_t s) {
  const int rows = a.bs ? a.nslots : 1;
  hipLaunchKernelGGL(k_top_slice, dim3((a.V + a.L - 1) / a.L, rows), dim3(TOPS_THREADS), 0, s, a);
  hipLaunchKernelGGL(k_top_merge, dim3(rows), dim3(TOPS_THREADS), 0, s, a);
}
