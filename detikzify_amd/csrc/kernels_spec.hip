// kernels_spec.hip — prompt-lookup speculative decoding inside the multi-vector step (dtk_spec_*).
//
// The verify pass of a speculative step is the multi-vector step itself: its 2 or 4 vectors are consecutive positions of ONE sequence
// (slot 0), all reading and writing slot 0's key/value cache.  Vector 0 forwards the last accepted token, vector i > 0 the draft d_i.
// Two small kernels (three with a corpus) sit between the step's sampler launch and its first GEMV:
//   k_spec_accept  one thread.  The sampler has left s_i, the token sampled from vector i's pending logits row, in the step's token
//                  record for every vector that was live in the previous step.  n = the number of leading i with vector i + 1 live and
//                  s_i == d_{i+1}: the tokens s_0 .. s_n are the sequence's next n + 1 tokens (what n + 1 plain steps sample).  The
//                  count goes to the record, the tokens to the device history, and slot 0's true DecState moves to the position, draw
//                  index and last token a plain decode would hold there.
//   k_spec_corpus  (only while dtk_spec_set_corpus holds a corpus of earlier programs) 64 blocks: one pass over the corpus for the window
//                  that matches the longest n-gram at the history's end, lowest index first; one result per block.
//   k_spec_draft   one block.  Drafts for the next positions — HF's PromptLookupCandidateGenerator over the device history, with the
//                  corpus window's continuation where the history has no window of that n-gram size, or the
//                  caller's table of ids per absolute position (tests decide acceptance with it) — then the vectors' DecStates, the
//                  gathered embeddings of [s_n, d_1 .. d_k] in the residual rows, and the active flags of the vectors without a draft
//                  cleared in the step's device BatchState so their GEMV lanes and attention blocks return at once.
// Everything is written with ordinary vector stores by the threads that hold the values; no atomics on global memory.
#include "kernels.h"

#define SPEC_THREADS 1024

namespace {

__global__ __launch_bounds__(64) void k_spec_accept(SpecArgs a) {
  if (threadIdx.x != 0) return;
  const size_t ri = (size_t)((unsigned)a.bs->step % (unsigned)a.ring) * DTK_MAX_BATCH;
  const int NV = a.sd->NV;
  int n = 0;
  while (n + 1 < NV && a.bs->active[n + 1] != 0 && a.tok_ring[ri + n] == (int64_t)a.sd->drafts[n + 1]) ++n;
  const int P = a.st_true->next_pos;          // the position s_0 takes
  int cnt = n + 1;
  if (P + cnt > a.T_max) cnt = a.T_max - P;   // (the host never launches a step that could get here: DTK_ERR_RANGE)
  if (cnt < 1) { a.tok_ring[ri + DTK_SPEC_COUNT_AT] = 0; return; }
  for (int i = 0; i < cnt; ++i) a.hist[P + i] = (int32_t)a.tok_ring[ri + i];
  a.tok_ring[ri + DTK_SPEC_COUNT_AT] = (int64_t)cnt;
  DecState st = *a.st_true;
  st.pos = P + cnt - 1;
  st.next_pos = P + cnt;
  st.token = (int32_t)a.tok_ring[ri + cnt - 1];
  st.draw = st.draw + (uint32_t)cnt;
  st.force_plus1 = 0;
  *a.st_true = st;
}

// The corpus pass: every block covers DTK_SPEC_CORPUS_THREADS consecutive entries, a thread owns one END position e of a window.  With
// c[e] equal to the tail's last id and a continuation id behind it (e + 1 < C, c[e + 1] >= 0; a separator is negative and no tail id is),
// L = how many ids backwards from e equal the tail's ids backwards from its end, capped at nmax: the window of n ids ending at e matches
// the last n ids for every n <= L.  The key (L << 32) | (0xffffffff - e) orders by the longest n-gram first and the lowest index among
// those; the block's maximum goes to the block's own entry of corpus_best with a plain store, so the result depends on no order among
// threads or blocks.  A block past the corpus returns after reading the length (k_spec_draft reads the entries in front of it only).
__global__ __launch_bounds__(DTK_SPEC_CORPUS_THREADS) void k_spec_corpus(SpecArgs a) {
  __shared__ int s_tail[DTK_SPEC_MAX_NGRAM];
  __shared__ unsigned long long s_best[DTK_SPEC_CORPUS_THREADS / 64];
  const int tid = threadIdx.x;
  const int C = a.sd->corpus_len;
  const int base = (int)blockIdx.x * DTK_SPEC_CORPUS_THREADS;
  if (base >= C) return;                         // (block-uniform)
  const int len = a.len_override >= 0 ? a.len_override : a.st_true->next_pos;
  int nmax = a.sd->max_ngram < DTK_SPEC_MAX_NGRAM ? a.sd->max_ngram : DTK_SPEC_MAX_NGRAM;
  if (nmax > len - 1) nmax = len - 1;
  if (nmax < 1) {                                // (block-uniform) no tail to match: k_spec_draft does not look either
    if (tid == 0) a.sd->corpus_best[blockIdx.x] = 0ull;
    return;
  }
  if (tid < nmax) s_tail[tid] = a.hist[len - nmax + tid];
  __syncthreads();
  const int32_t* c = a.sd->corpus;
  const int e = base + tid;
  unsigned long long key = 0ull;
  if (e + 1 < C && c[e] == s_tail[nmax - 1] && c[e + 1] >= 0) {
    int L = 1;
    while (L < nmax && e - L >= 0 && c[e - L] == s_tail[nmax - 1 - L]) ++L;
    key = ((unsigned long long)L << 32) | (unsigned long long)(0xffffffffu - (unsigned)e);
  }
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off, 64);
    key = o > key ? o : key;
  }
  if ((tid & 63) == 0) s_best[tid >> 6] = key;
  __syncthreads();
  if (tid < 64) {
    key = tid < DTK_SPEC_CORPUS_THREADS / 64 ? s_best[tid] : 0ull;
    for (int off = 8; off >= 1; off >>= 1) {
      const unsigned long long o = __shfl_xor(key, off, 64);
      key = o > key ? o : key;
    }
    if (tid == 0) a.sd->corpus_best[blockIdx.x] = key;
  }
}

// the drafts for a history of len ids: d[0 .. k), k <= kmax (every thread of the block calls it; s_idx / s_d / s_from are LDS).  At every
// n the sequence's own history is searched first (HF's rule); the corpus supplies the drafts at n == n_c, the longest n-gram for which
// k_spec_corpus found a window (ending at e_c, a continuation id behind it), when the history has no window of that size.
// s_from[0] = DTK_SPEC_FROM_*, s_from[1] = the n that matched (0: none)
__device__ __forceinline__ int spec_lookup(const int32_t* hist, int len, int kmax, int max_ngram, const int32_t* corpus, int C, int n_c, int e_c,
                                           int* s_idx, int* s_d, int* s_from) {
  const int tid = threadIdx.x;
  int k = 0;
  int n = max_ngram < len - 1 ? max_ngram : len - 1;
  for (; n >= 1 && kmax > 0; --n) {              // (block-uniform loop: n, kmax and the LDS word are the same for every thread)
    if (tid == 0) *s_idx = 0x7fffffff;
    __syncthreads();
    const int32_t* tail = hist + (len - n);
    int mine = 0x7fffffff;
    for (int idx = tid; idx < len - n && mine == 0x7fffffff; idx += SPEC_THREADS) {
      bool eq = true;
      for (int j = 0; j < n && eq; ++j) eq = hist[idx + j] == tail[j];
      if (eq) mine = idx;
    }
    if (mine != 0x7fffffff) atomicMin(s_idx, mine);      // (an LDS word)
    __syncthreads();
    const int first = *s_idx;
    __syncthreads();
    if (first != 0x7fffffff) {
      const int start = first + n;               // <= len - 1: the continuation holds at least one id
      k = len - start < kmax ? len - start : kmax;
      if (tid < k) s_d[tid] = hist[start + tid];
      if (tid == 0) { s_from[0] = DTK_SPEC_FROM_HISTORY; s_from[1] = n; }
      __syncthreads();
      break;
    }
    if (n == n_c) {                              // c[e_c + 1] is an id (k_spec_corpus): cut in front of the first separator or at C
      if (tid == 0) {
        int kc = 0;
        while (kc < kmax && e_c + 1 + kc < C && corpus[e_c + 1 + kc] >= 0) { s_d[kc] = corpus[e_c + 1 + kc]; ++kc; }
        *s_idx = kc; s_from[0] = DTK_SPEC_FROM_CORPUS; s_from[1] = n;
      }
      __syncthreads();
      k = *s_idx;
      break;
    }
  }
  return k;
}

__global__ __launch_bounds__(SPEC_THREADS) void k_spec_draft(SpecArgs a) {
  __shared__ int s_idx;
  __shared__ int s_d[4];
  __shared__ int s_k;
  __shared__ int s_from[2];
  __shared__ unsigned long long s_best;
  const int tid = threadIdx.x;
  const int len = a.len_override >= 0 ? a.len_override : a.st_true->next_pos;     // ids in the history; the last one is forwarded by vector 0
  const int p = len - 1;
  // the sequence's own settings live in device memory (dtk_spec_begin writes them): a captured step serves every K, n-gram size and source
  const int K = a.sd ? a.sd->K : a.K, NV = a.sd ? a.sd->NV : a.NV, max_ngram = a.sd ? a.sd->max_ngram : a.max_ngram;
  const bool from_table = a.sd && a.sd->use_table != 0;
  const int C = a.sd && !from_table ? a.sd->corpus_len : 0;      // (the table source ignores the corpus)
  int kmax = K;
  if (kmax > a.T_max - 1 - p) kmax = a.T_max - 1 - p;      // no vector's position reaches T_max
  if (kmax > NV - 1) kmax = NV - 1;
  if (kmax > 3) kmax = 3;
  if (kmax < 0) kmax = 0;
  if (tid == 0) { s_from[0] = DTK_SPEC_FROM_NONE; s_from[1] = 0; }
  if (tid < 64) {                // k_spec_corpus's block results in front of the corpus end -> the best window of the whole corpus
    const int nb = (C + DTK_SPEC_CORPUS_THREADS - 1) / DTK_SPEC_CORPUS_THREADS;      // <= DTK_SPEC_CORPUS_BLOCKS = 64
    unsigned long long key = tid < nb ? a.sd->corpus_best[tid] : 0ull;
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned long long o = __shfl_xor(key, off, 64);
      key = o > key ? o : key;
    }
    if (tid == 0) s_best = key;
  }
  __syncthreads();
  const int n_c = (int)(s_best >> 32), e_c = (int)(0xffffffffu - (unsigned)(s_best & 0xffffffffull));      // n_c = 0: no window anywhere
  int k = 0;
  if (from_table) {
    if (tid == 0) {
      while (k < kmax) {
        const int32_t t = a.table[p + 1 + k];
        if (t < 0 || t >= a.V) break;
        s_d[k++] = t;
      }
      s_k = k;
      if (k) s_from[0] = DTK_SPEC_FROM_HISTORY;
    }
    __syncthreads();
    k = s_k;
  } else if (len >= 2) {
    k = spec_lookup(a.hist, len, kmax, max_ngram, C ? a.sd->corpus : nullptr, C, n_c, e_c, &s_idx, s_d, s_from);
  }
  if (a.drafts_out) {          // the op entry point: the drafts, their count, their source and the n-gram size alone
    if (tid < 4) a.drafts_out[tid] = tid < k ? s_d[tid] : -1;
    if (tid == 0) a.drafts_out[4] = k;
    if (tid == 1) a.drafts_out[5] = s_from[0];
    if (tid == 2) a.drafts_out[6] = s_from[1];
    return;
  }
  const int32_t last = a.hist[p];
  const uint32_t c = a.st_true->draw;
  if (tid < 4) {
    const int j = tid;
    const bool live = j <= k && j < NV;
    const int32_t tok = (j >= 1 && live) ? s_d[j - 1] : last;
    DecState st{};
    st.pos = live ? p + j : p;          // a vector without a draft is skipped by every kernel; its record still points inside the cache
    st.next_pos = st.pos + 1;
    st.token = tok;
    st.draw = c + (uint32_t)j;
    a.st_vec[j] = st;
    a.sd->drafts[j] = live ? tok : -1;
    a.bs->active[j] = live ? 1 : 0;
  }
  if (tid == 4) a.bs->step = (int32_t)(((unsigned)a.bs->step + 1u) % (unsigned)a.ring);      // the record index of the next step
  if (tid == 5) a.sd->n_live = k + 1;
  if (tid == 6) a.sd->steps[s_from[0]] += 1;      // (one thread of one block per step: a plain read and store)
  // the embeddings of [s_n, d_1 .. d_k]: the first operation of the forward that follows
  const int chunks = a.d >> 3;
  for (int j = 0; j <= k && j < NV; ++j) {
    const int32_t tok = j ? s_d[j - 1] : last;
    const u32x4* src = reinterpret_cast<const u32x4*>(a.embed + (size_t)tok * a.d);
    u32x4* dst = reinterpret_cast<u32x4*>(a.x + (size_t)j * a.d);
    for (int q = tid; q < chunks; q += SPEC_THREADS) dst[q] = src[q];
  }
}

}  // namespace

void launch_spec_accept(const SpecArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_spec_accept, dim3(1), dim3(64), 0, s, a); }
void launch_spec_corpus(const SpecArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_spec_corpus, dim3(DTK_SPEC_CORPUS_BLOCKS), dim3(DTK_SPEC_CORPUS_THREADS), 0, s, a);
}
void launch_spec_draft(const SpecArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_spec_draft, dim3(1), dim3(SPEC_THREADS), 0, s, a); }
