// dtk_ops.hip — the op-level test entry points of the C ABI (include/dtk.h: dtk_op_*, dtk_mx_layout, dtk_w13_*_host): one kernel or
// one launcher of the product on host operands, staged through the context's op scratch.  Test surface only: nothing here runs in a
// prefill, a decode step or a sampler, and no kernel lives here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <vector>

#include "dtk_ctx.h"
#include "w13.h"
#include "mx_quant.h"

// the library is built with -fvisibility=hidden: the C ABI of include/dtk.h is all it exports
#pragma GCC visibility push(default)
extern "C" {

// ---- staging: every op puts its host operands into the context's op scratch through one OpRun.  in<T>() declares an operand, io<T>() a
// result that is uploaded first (in/out), out<T>() a result that is only read back, take() device room of the op's own; then upload()
// once, the launches, finish().  fill = a byte (the ops with a scratch_fill argument): the whole scratch the op uses is filled with it
// first and the 256 guard bytes behind every result must still hold it after the launches.  fill = -1 (the ops without one): nothing is
// filled, no guard bytes are reserved and none are checked.
extern "C++" {
namespace {
struct OpRun {
  static constexpr size_t GUARD = 256;
  dtk_ctx* c; const char* who; int fill; size_t off = 0, need = 0; bool full = false;
  struct In { void* dev; const void* host; size_t bytes; };
  struct Res { void* dev; void* host; size_t bytes; const char* name; bool up; };
  std::vector<In> ins; std::vector<Res> res;
  OpRun(dtk_ctx* c_, const char* who_, int fill_ = -1) : c(c_), who(who_), fill(fill_) {}
  void* take(size_t bytes) {
    off = align_up(off, 256);
    if (off + bytes + (fill < 0 ? 0 : 256) > c->scratch_bytes) { if (!full) need = off + bytes; full = true; return c->scratch; }
    void* p = c->scratch + off; off += bytes; return p;
  }
  template <class T> T* result(void* host, size_t n, const char* name, bool up) {
    T* p = (T*)take(n * sizeof(T) + (fill < 0 ? 0 : GUARD));
    res.push_back({p, host, n * sizeof(T), name, up});      // (no host buffer: nothing is copied, the guard is still checked)
    return p;
  }
  template <class T> T* in(const void* host, size_t n) { T* p = (T*)take(n * sizeof(T)); if (host && n) ins.push_back({p, host, n * sizeof(T)}); return p; }
  template <class T> T* io(void* host, size_t n, const char* name) { return result<T>(host, n, name, true); }
  template <class T> T* out(void* host, size_t n, const char* name) { return result<T>(host, n, name, false); }
  int upload(hipStream_t s) {     // the caller's poison over everything between and behind the operands, then the operands
    if (full && fill < 0) return fail(c, DTK_ERR_ARG, "op scratch exhausted (%zu bytes)", need);
    if (full) return fail(c, DTK_ERR_ARG, "%s: op scratch exhausted (%zu of %zu bytes)", who, off, c->scratch_bytes);
    off = align_up(off, 256);
    if (fill >= 0) HIPCHK(c, hipMemsetAsync(c->scratch, fill, off + 256, s));
    for (const In& i : ins) HIPCHK(c, hipMemcpyAsync(i.dev, i.host, i.bytes, hipMemcpyHostToDevice, s));
    for (const Res& r : res) if (r.up && r.host && r.bytes) HIPCHK(c, hipMemcpyAsync(r.dev, r.host, r.bytes, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));      // (host temporaries handed to in() live until here)
    return DTK_OK;
  }
  int finish(hipStream_t s) {     // nothing behind the end of a result buffer was written; then the results go back
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    unsigned char guard[GUARD];
    for (const Res& r : res) {
      if (fill < 0) break;
      HIPCHK(c, hipMemcpy(guard, (unsigned char*)r.dev + r.bytes, GUARD, hipMemcpyDeviceToHost));
      for (size_t j = 0; j < GUARD; ++j)
        if (guard[j] != (unsigned char)fill) return fail(c, DTK_ERR_STATE, "%s: byte %zu behind the end of %s was written", who, j, r.name);
    }
    for (const Res& r : res) if (r.host && r.bytes) HIPCHK(c, hipMemcpy(r.host, r.dev, r.bytes, hipMemcpyDeviceToHost));
    return DTK_OK;
  }
};

inline std::vector<int32_t> ids32_of(const int64_t* ids, int n) {      // token ids as the kernels hold them
  std::vector<int32_t> v((size_t)(n > 0 ? n : 0));
  for (int i = 0; i < n; ++i) v[(size_t)i] = (int32_t)ids[i];
  return v;
}
inline size_t host_xtile_off(int slot, int k, int nsteps) {      // xtile_off (common.h): where element k of slot `slot` lies in a fragment-major buffer
  return ((size_t)((slot >> 4) * nsteps + (k >> 5)) * 64 + ((k & 31) >> 3) * 16 + (slot & 15)) * 8 + (k & 7);
}
}  // namespace
}  // extern "C++"


int dtk_op_gemm(dtk_ctx* c, const uint16_t* A, const uint16_t* W, const uint16_t* bias, const uint16_t* residual, int M, int N, int K, int flags, uint16_t* C) {
  if (!c || !A || !W || !C || K % 8) return fail(c, DTK_ERR_ARG, "dtk_op_gemm: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const bool has_bias = (flags & (DTK_EPI_BIAS | DTK_EPI_GELU)) && bias, has_res = (flags & DTK_EPI_RESIDUAL) && residual;
  const int S = (flags >> DTK_GEMM_KSLICES_SHIFT) & 15;       // 0 = a one-chain GEMM; 1..8 = the sliced-K family (1: one slice through the partial + reduce path)
  OpRun r(c, "dtk_op_gemm");
  GemmArgs g;
  g.A = r.in<bf16_t>(A, (size_t)M * K); g.lda = K; g.W = r.in<bf16_t>(W, (size_t)N * K); g.ldw = K;
  g.bias = r.in<bf16_t>(has_bias ? bias : nullptr, N);
  g.residual = r.in<bf16_t>(has_res ? residual : nullptr, (size_t)M * N); g.ldr = N;
  g.C = r.out<bf16_t>(C, (size_t)M * N, "C"); g.ldc = N;
  g.M = M; g.N = N; g.K = K;
  g.flags = (has_bias ? GEMM_BIAS : 0) | ((flags & DTK_EPI_GELU) ? gelu_flag(c) : 0) | (has_res ? GEMM_RESIDUAL : 0);
  // + the fragment-major copy of W (k_gemm_g3's W stage is filled from it)
  bf16_t* dWt = (flags & DTK_GEMM_WT) ? (bf16_t*)r.take(tiled_elems(N, K) * sizeof(bf16_t)) : nullptr;
  if (r.full) return r.upload(s);
  if (S > 8) return fail(c, DTK_ERR_ARG, "dtk_op_gemm: at most 8 K slices");
  if (S) g.kslices = S;
  if (S && !(flags & DTK_GEMM_NAIVE)) { g.part = (float*)r.take((size_t)S * M * N * sizeof(float)); g.part_stride = (long)M * N; }
  if (const int rc = r.upload(s)) return rc;
  if (dWt) { launch_retile(g.W, dWt, N, K, s); g.Wt = dWt; }
  if (S) {
    if (flags & DTK_GEMM_NAIVE) launch_gemm_naive(g, s);
    else if (flags & DTK_GEMM_SL) { if (!launch_gemm_g3_sliced(g, s)) return fail(c, DTK_ERR_ARG, "dtk_op_gemm: the in-register sliced kernel does not take this shape"); }
    else if (!launch_gemm_sk(g, nullptr, nullptr, 0, 0.f, s)) return fail(c, DTK_ERR_ARG, "dtk_op_gemm: the sliced-K kernel does not take this shape");
  }
  else if (flags & DTK_GEMM_NAIVE) launch_gemm_naive(g, s); else launch_gemm_mfma(g, s);
  return r.finish(s);
}

int dtk_gemm_last_kernel(void) { return gemm_last_kernel(); }

// One GEMM launch as the product makes it: strided operands, bias / residual / C at element offsets inside their buffers (a pointer that is
// 2-, 4- or 8-byte aligned only), the residual in place, either GELU whatever the context's config.  c_io is IN/OUT: what the kernel leaves
// alone keeps the caller's bits; guard bytes behind it; *kernel_out = the launchers' record (kernels.h: GEMM_KCODE).
int dtk_op_gemm_ex(dtk_ctx* c, const uint16_t* A, int64_t na, const uint16_t* W, int64_t nw, const uint16_t* bias, int64_t nb,
                   const uint16_t* residual, int64_t nr, const uint16_t* gate, uint16_t* c_io, int64_t nc, int M, int N, int K,
                   int lda, int ldw, int ldr, int ldc, int b_off, int r_off, int c_off, int flags, int scratch_fill, int* kernel_out) {
  const char* who = "dtk_op_gemm_ex";
  if (!c) return DTK_ERR_ARG;
  if (!A || !W || !c_io) return fail(c, DTK_ERR_ARG, "%s: A, W and c_io required", who);
  if (M < 1 || N < 1 || K < 8 || (K % 8) || scratch_fill < 0 || scratch_fill > 255) return fail(c, DTK_ERR_ARG, "%s: M, N >= 1, K a multiple of 8, scratch_fill a byte", who);
  if (b_off < 0 || r_off < 0 || c_off < 0 || na < 1 || nw < 1 || nc < 1) return fail(c, DTK_ERR_ARG, "%s: negative offset or empty buffer", who);
  const int known = DTK_EPI_BIAS | DTK_EPI_GELU | DTK_EPI_RESIDUAL | DTK_EPI_GATED_RESIDUAL | DTK_EPI_GELU_ERF | DTK_EPI_GELU_TANH | DTK_GEMM_INPLACE |
                    DTK_GEMM_NAIVE | DTK_GEMM_WT | DTK_GEMM_SL | (15 << DTK_GEMM_KSLICES_SHIFT);
  if (flags & ~known) return fail(c, DTK_ERR_ARG, "%s: unknown flag bits %#x", who, flags & ~known);
  const bool has_bias = (flags & DTK_EPI_BIAS) != 0, has_res = (flags & DTK_EPI_RESIDUAL) != 0, inplace = (flags & DTK_GEMM_INPLACE) != 0;
  const bool gated = (flags & DTK_EPI_GATED_RESIDUAL) != 0;
  const int ngelu = ((flags & DTK_EPI_GELU) != 0) + ((flags & DTK_EPI_GELU_ERF) != 0) + ((flags & DTK_EPI_GELU_TANH) != 0);
  const int S = (flags >> DTK_GEMM_KSLICES_SHIFT) & 15;
  if (ngelu > 1) return fail(c, DTK_ERR_ARG, "%s: one GELU at most", who);
  if (has_bias && !bias) return fail(c, DTK_ERR_ARG, "%s: DTK_EPI_BIAS without a bias", who);
  if (inplace && (!has_res || residual)) return fail(c, DTK_ERR_ARG, "%s: DTK_GEMM_INPLACE needs DTK_EPI_RESIDUAL and residual = NULL (c_io holds it)", who);
  if (has_res && !inplace && !residual) return fail(c, DTK_ERR_ARG, "%s: DTK_EPI_RESIDUAL without a residual", who);
  if (gated && (!has_res || !gate)) return fail(c, DTK_ERR_ARG, "%s: DTK_EPI_GATED_RESIDUAL needs DTK_EPI_RESIDUAL and a gate", who);
  if (S > 8) return fail(c, DTK_ERR_ARG, "%s: at most 8 K slices", who);
  if ((flags & DTK_GEMM_SL) && S < 2) return fail(c, DTK_ERR_ARG, "%s: DTK_GEMM_SL needs 2..8 K slices", who);
  if ((lda % 8) || (ldw % 8) || lda < K || ldw < K) return fail(c, DTK_ERR_ARG, "%s: A and W rows are 16-byte aligned: lda (%d), ldw (%d) multiples of 8 and >= K", who, lda, ldw);
  if (ldc < N || (has_res && !inplace && ldr < N)) return fail(c, DTK_ERR_ARG, "%s: ldc (%d) / ldr (%d) below N", who, ldc, ldr);
  if ((int64_t)(M - 1) * lda + K > na) return fail(c, DTK_ERR_ARG, "%s: the strides of A address element %lld of %lld", who, (long long)((int64_t)(M - 1) * lda + K), (long long)na);
  if ((int64_t)(N - 1) * ldw + K > nw) return fail(c, DTK_ERR_ARG, "%s: the strides of W address element %lld of %lld", who, (long long)((int64_t)(N - 1) * ldw + K), (long long)nw);
  if (has_bias && (int64_t)b_off + N > nb) return fail(c, DTK_ERR_ARG, "%s: the offset of bias addresses element %lld of %lld", who, (long long)((int64_t)b_off + N), (long long)nb);
  if (has_res && !inplace && (int64_t)r_off + (int64_t)(M - 1) * ldr + N > nr)
    return fail(c, DTK_ERR_ARG, "%s: the strides of residual address element %lld of %lld", who, (long long)((int64_t)r_off + (int64_t)(M - 1) * ldr + N), (long long)nr);
  if ((int64_t)c_off + (int64_t)(M - 1) * ldc + N > nc)
    return fail(c, DTK_ERR_ARG, "%s: the strides of C address element %lld of %lld", who, (long long)((int64_t)c_off + (int64_t)(M - 1) * ldc + N), (long long)nc);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  std::vector<bf16_t> packed;      // DTK_GEMM_WT: launch_retile reads contiguous rows
  if ((flags & DTK_GEMM_WT) && ldw != K) {
    packed.resize((size_t)N * K);
    for (int n = 0; n < N; ++n) memcpy(packed.data() + (size_t)n * K, W + (size_t)n * ldw, (size_t)K * 2);
  }
  OpRun r(c, who, scratch_fill);
  GemmArgs g;
  g.A = r.in<bf16_t>(A, (size_t)na); g.lda = lda; g.W = r.in<bf16_t>(W, (size_t)nw); g.ldw = ldw;
  const bf16_t* dB = r.in<bf16_t>(has_bias ? bias : nullptr, has_bias ? (size_t)nb : 0);
  const bf16_t* dR = r.in<bf16_t>(has_res && !inplace ? residual : nullptr, has_res && !inplace ? (size_t)nr : 0);
  g.gate = r.in<bf16_t>(gated ? gate : nullptr, gated ? 1 : 0);
  bf16_t* dC = r.io<bf16_t>(c_io, (size_t)nc, "C");
  g.bias = has_bias ? dB + b_off : nullptr;
  g.C = dC + c_off; g.ldc = ldc;
  g.residual = !has_res ? nullptr : (inplace ? g.C : dR + r_off); g.ldr = inplace ? ldc : ldr;
  g.M = M; g.N = N; g.K = K;
  g.flags = (has_bias ? GEMM_BIAS : 0) | ((flags & DTK_EPI_GELU) ? gelu_flag(c) : 0) | ((flags & DTK_EPI_GELU_ERF) ? GEMM_GELU_ERF : 0) |
            ((flags & DTK_EPI_GELU_TANH) ? GEMM_GELU_TANH : 0) | (has_res ? GEMM_RESIDUAL : 0) | (gated ? GEMM_GATED_RESIDUAL : 0);
  const bf16_t* dWp = packed.empty() ? g.W : r.in<bf16_t>(packed.data(), packed.size());
  bf16_t* dWt = (flags & DTK_GEMM_WT) ? (bf16_t*)r.take(tiled_elems(N, K) * sizeof(bf16_t)) : nullptr;
  if (S) g.kslices = S;
  const bool sliced_mfma = S && !(flags & DTK_GEMM_NAIVE);
  if (sliced_mfma && !(flags & DTK_GEMM_SL)) { g.part = (float*)r.take((size_t)S * M * N * sizeof(float)); g.part_stride = (long)M * N; }
  if (r.full) return r.upload(s);
  if (sliced_mfma && !gemm_sk_supported(g))      // (asked before anything is uploaded)
    return fail(c, DTK_ERR_ARG, "%s: the sliced-K kernels need K >= 128 and N %% 4 == 0", who);
  if (const int rc = r.upload(s)) return rc;
  if (dWt) { launch_retile(dWp, dWt, N, K, s); g.Wt = dWt; }
  if (flags & DTK_GEMM_NAIVE) launch_gemm_naive(g, s);
  else if (S && (flags & DTK_GEMM_SL)) { if (!launch_gemm_g3_sliced(g, s)) return fail(c, DTK_ERR_ARG, "%s: the in-register sliced kernel does not take this shape", who); }
  else if (S) { if (!launch_gemm_sk(g, nullptr, nullptr, 0, 0.f, s)) return fail(c, DTK_ERR_ARG, "%s: the sliced-K kernel does not take this shape", who); }
  else launch_gemm_mfma(g, s);
  if (kernel_out) *kernel_out = gemm_last_kernel();
  return r.finish(s);
}

int dtk_op_score(dtk_ctx* c, const uint16_t* Xn, const uint16_t* W, const int32_t* targets, int M, int N, int K, int flags,
                 float* logprob_out, float* lse_out, int32_t* argmax_out, float* zmax_out) {
  return dtk_op_score_top(c, Xn, W, targets, M, N, K, flags, logprob_out, lse_out, argmax_out, zmax_out, 0, nullptr, nullptr, nullptr);
}

int dtk_op_score_top(dtk_ctx* c, const uint16_t* Xn, const uint16_t* W, const int32_t* targets, int M, int N, int K, int flags,
                     float* logprob_out, float* lse_out, int32_t* argmax_out, float* zmax_out, int k, int32_t* top_ids_out,
                     float* top_logprob_out, float* top_z_out) {
  if (!c || !Xn || !W || !targets || !logprob_out || M < 1 || N < 1 || K < 8 || K % 8) return fail(c, DTK_ERR_ARG, "dtk_op_score: bad argument");
  if (k != 0 || top_ids_out || top_logprob_out || top_z_out) {
    if (k < 1 || k > DTK_MAX_TOP || k > N) return fail(c, DTK_ERR_ARG, "dtk_op_score_top: k = %d (1 .. min(DTK_MAX_TOP = %d, N), or 0 with NULL outputs)", k, DTK_MAX_TOP);
    if (!top_ids_out || !top_logprob_out) return fail(c, DTK_ERR_ARG, "dtk_op_score_top: k = %d needs top_ids_out and top_logprob_out", k);
  }
  for (int m = 0; m < M; ++m)
    if (targets[m] < 0 || targets[m] >= N) return fail(c, DTK_ERR_ARG, "dtk_op_score: target %d of row %d outside [0, %d)", targets[m], m, N);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t mk = (size_t)M * k;
  OpRun r(c, "dtk_op_score", 0xFF);     // the records start as NaN (a record the kernels leave out shows), guard bytes behind every result
  GemmArgs g;
  g.A = r.in<bf16_t>(Xn, (size_t)M * K); g.lda = K; g.W = r.in<bf16_t>(W, (size_t)N * K); g.ldw = K;
  g.bias = nullptr; g.residual = nullptr; g.ldr = 0; g.C = nullptr; g.ldc = 0;
  g.M = M; g.N = N; g.K = K; g.flags = 0; g.ls_target = r.in<int32_t>(targets, M);
  float* dRec = (float*)r.take(score_rec_floats(M, N) * sizeof(float));
  g.ls_rec = dRec;
  float* dlp = r.out<float>(logprob_out, M, "logprob"); float* dlse = r.out<float>(lse_out, M, "lse");
  int32_t* dam = r.out<int32_t>(argmax_out, M, "argmax"); float* dz = r.out<float>(zmax_out, M, "zmax");
  int32_t* dti = r.out<int32_t>(top_ids_out, mk, "top_ids"); float* dtl = r.out<float>(top_logprob_out, mk, "top_logprob");
  float* dtz = r.out<float>(top_z_out, mk, "top_z");
  bf16_t* dWt = (flags & DTK_GEMM_WT) ? (bf16_t*)r.take(tiled_elems(N, K) * sizeof(bf16_t)) : nullptr;
  if (const int rc = r.upload(s)) return rc;
  if (dWt) { launch_retile(g.W, dWt, N, K, s); g.Wt = dWt; }
  if (!launch_gemm_logsoftmax(g, s)) return fail(c, DTK_ERR_ARG, "dtk_op_score: the kernel does not take this shape");
  launch_score_merge(dRec, M, N, dlp, dlse, dam, dz, s);
  if (k > 0) launch_score_top(g, dlse, k, dti, dtl, dtz, s);
  return r.finish(s);
}

int dtk_op_gemm_gated(dtk_ctx* c, const uint16_t* A, const uint16_t* W, const uint16_t* bias, const uint16_t* residual,
                      const uint16_t* gate, int M, int N, int K, int flags, uint16_t* C) {
  if (!c || !A || !W || !C || !bias || !residual || !gate || K % 8) return fail(c, DTK_ERR_ARG, "dtk_op_gemm_gated: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, "dtk_op_gemm_gated");
  GemmArgs g;
  g.A = r.in<bf16_t>(A, (size_t)M * K); g.lda = K; g.W = r.in<bf16_t>(W, (size_t)N * K); g.ldw = K;
  g.bias = r.in<bf16_t>(bias, N); g.residual = r.in<bf16_t>(residual, (size_t)M * N); g.ldr = N;
  g.C = r.out<bf16_t>(C, (size_t)M * N, "C"); g.ldc = N;
  g.gate = r.in<bf16_t>(gate, 1);
  g.M = M; g.N = N; g.K = K; g.flags = GEMM_BIAS | GEMM_RESIDUAL | GEMM_GATED_RESIDUAL;
  if (const int rc = r.upload(s)) return rc;
  if (flags & DTK_GEMM_NAIVE) launch_gemm_naive(g, s); else launch_gemm_mfma(g, s);
  return r.finish(s);
}

int dtk_op_gemv(dtk_ctx* c, const uint16_t* W, const uint16_t* x, const uint16_t* norm_w, int N, int K, int mode, float eps, uint16_t* y) {
  if (!c || !W || !x || !y || K % 8) return fail(c, DTK_ERR_ARG, "dtk_op_gemv: bad argument");
  if (mode == 1 && !norm_w) return fail(c, DTK_ERR_ARG, "norm_w required");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, "dtk_op_gemv");
  GemvArgs g{};
  g.W = r.in<bf16_t>(W, (size_t)N * K); g.N = N; g.K = K; g.x = r.in<bf16_t>(x, K);
  g.norm_w = r.in<bf16_t>(mode == 1 ? norm_w : nullptr, K); g.eps = eps; g.y = r.out<bf16_t>(y, N, "y");
  if (const int rc = r.upload(s)) return rc;
  launch_gemv(mode == 1 ? PRO_RMSNORM : PRO_COPY, EPI_STORE, g, s);
  return r.finish(s);
}

// The MXFP4 GEMV on host buffers: W [N][K] row-major bf16 goes through the shipped quantiser (launch_quant_mxfp4_rows) and the shipped
// launch_gemv with EPI_STORE (mode 0: y = W_eff . x, mode 1: y = W_eff . rmsnorm(x, norm_w)); w_eff_out (optional, [N][K]) receives the
// de-quantised weights the kernel computed with.  Any context serves (the op brings its own weights).
int dtk_op_gemv_q4(dtk_ctx* c, const uint16_t* W, const uint16_t* x, const uint16_t* norm_w, int N, int K, int mode, float eps, uint16_t* y, uint16_t* w_eff_out) {
  if (!c || !W || !x || !y || N < 1 || K < 8 || (K % 8) || (mode != 0 && mode != 1) || (mode == 1 && !norm_w)) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_q4: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t nw = (size_t)N * K;
  OpRun r(c, "dtk_op_gemv_q4");
  // the quantiser leaves the de-quantised weights in place of W: with w_eff_out the rows are an in/out result that starts as W
  if (w_eff_out) memmove(w_eff_out, W, nw * 2);
  bf16_t* dW = w_eff_out ? r.io<bf16_t>(w_eff_out, nw, "w_eff") : r.in<bf16_t>(W, nw);
  GemvArgs g{};
  g.W = dW; g.N = N; g.K = K; g.x = r.in<bf16_t>(x, K); g.norm_w = r.in<bf16_t>(mode == 1 ? norm_w : nullptr, K); g.eps = eps;
  g.y = r.out<bf16_t>(y, N, "y");
  uint8_t* dQ = (uint8_t*)r.take((size_t)N * mxfp4_row_bytes(K)); uint8_t* dS = (uint8_t*)r.take((size_t)N * mxfp4_row_scales(K));
  g.W4 = dQ; g.S4 = dS;
  if (const int rc = r.upload(s)) return rc;
  launch_quant_mxfp4_rows(dW, dQ, dS, N, K, s);
  launch_gemv(mode == 1 ? PRO_RMSNORM : PRO_COPY, EPI_STORE, g, s);
  return r.finish(s);
}

// nb (1, 2 or 4) input vectors through k_gemv_mv: y[b] = W . x[b] (mode 0) or W . rmsnorm(x[b], norm_w) (mode 1); per vector
// the result must equal dtk_op_gemv's bit for bit (same lane / chunk order, same wave reduction, same block size)
int dtk_op_gemv_mv(dtk_ctx* c, const uint16_t* W, const uint16_t* X, const uint16_t* norm_w, int N, int K, int mode, float eps, int nb, uint16_t* Y) {
  if (!c || !W || !X || !Y || N < 1 || K < 8 || (K & 7) || (nb != 1 && nb != 2 && nb != 4) || (mode == 1 && !norm_w))
    return fail(c, DTK_ERR_ARG, "dtk_op_gemv_mv: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, "dtk_op_gemv_mv");
  GemvMvArgs g{};
  g.W = r.in<bf16_t>(W, (size_t)N * K); g.N = N; g.K = K; g.X = r.in<bf16_t>(X, (size_t)nb * K); g.ldx = K; g.x_rowmajor = 1;
  g.norm_w = r.in<bf16_t>(norm_w, K); g.eps = eps; g.Y = r.out<bf16_t>(Y, (size_t)nb * N, "Y"); g.ldy = N; g.d = K; g.ff = N;
  if (const int rc = r.upload(s)) return rc;
  launch_gemv_mv(mode == 1 ? PRO_RMSNORM : PRO_COPY, EPI_STORE, nb, g, s);
  return r.finish(s);
}

// Where value k of slot `slot` and the E8M0 scale of its group live in the MXFP8 buffers (csrc/mx_quant.h): pure host arithmetic (no
// GPU, no context) — tests/test_mx_layout.py checks on the CPU that this fragment order is the inverse of the operand map the
// instruction was measured to have.
int dtk_mx_layout(int G, int slot, int k, int64_t* data_off, int64_t* scale_off) {
  if ((G != 32 && G != 16) || slot < 0 || slot >= DTK_MAX_BATCH || k < 0 || !data_off || !scale_off) return DTK_ERR_ARG;
  *data_off = (int64_t)(G == 32 ? mx32_off(slot, k) : mx16_off(slot, k));
  *scale_off = (int64_t)(G == 32 ? mx32_soff(slot, k) : mx16_soff(slot, k));
  return DTK_OK;
}

// The fp8 matrix-core GEMVs of kernels_batch_mx.hip on host buffers.  W8 [N][K] e4m3 bytes + wscale [N]; X [nslots][K] bf16 rows,
// quantised to MXFP8 (groups of G = 32 | 16) by the step's own quantiser; nslots = 16 | 32 | 64 (1 / 2 / 4 slot tiles).
//   mode 0: unit kernel, logits epilogue (G = 32): Y [nslots][N] = bf16-rounded acc * wscale
//   mode 1: K-slice kernel of the N = d roles: Y [nslots][N] = the 8 slice partials added in order (fp32)
//   mode 2: unit kernel, SwiGLU epilogue (G = 32 in, N = 2 ff): y8_out / ys_out = the activation as MXFP8 groups of 16 (mx_x_bytes(ff, 16) / mx_s_bytes)
// x8_out / xs_out (optional): the quantised input as the kernels read it.
int dtk_op_gemv_mx(dtk_ctx* c, const uint8_t* W8, const float* wscale, const uint16_t* X, int N, int K, int G, int nslots, int mode,
                   float* Y, uint8_t* x8_out, uint8_t* xs_out, uint8_t* y8_out, uint8_t* ys_out) {
  if (!c || !W8 || !wscale || !X || (G != 32 && G != 16) || (nslots != 16 && nslots != 32 && nslots != 64) || mode < 0 || mode > 2)
    return fail(c, DTK_ERR_ARG, "dtk_op_gemv_mx: bad argument");
  if (mode != 1 && (G != 32 || !mx_unit_covers(K) || (N & 31))) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_mx: unit kernel needs G = 32, K %% 512 == 0, N %% 32 == 0");
  if (mode == 1 && !mx_kparts_covers(N, K, G)) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_mx: N = %d, K = %d, G = %d is not covered by the K-slice kernel", N, K, G);
  if ((mode != 2 && !Y) || (mode == 2 && (!y8_out || !ys_out || (N & 127)))) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_mx: missing output");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int ff = N / 2;
  const size_t ny = (size_t)(mode == 1 ? 8 : 1) * 64 * N;
  BatchState hbs; memset(&hbs, 0, sizeof hbs);
  for (int i = 0; i < nslots; ++i) hbs.active[i] = 1;
  for (int i = 0; i < DTK_MAX_BATCH; ++i) hbs.share_src[i] = -1;
  std::vector<bf16_t> hx((size_t)64 * K, (bf16_t)0);      // the 64 slots' rows: zero beyond nslots
  memcpy(hx.data(), X, (size_t)nslots * K * 2);
  std::vector<float> hy(mode == 2 ? 0 : ny);               // all the kernel's rows (mode 1: the 8 slices' partials)
  OpRun r(c, "dtk_op_gemv_mx");
  const uint8_t* dW = r.in<uint8_t>(W8, (size_t)N * K);
  uint8_t* dWm = (uint8_t*)r.take(mx_w_bytes(N, K, G));
  GemvBArgs g{};
  g.Wm = dWm; g.wscale = r.in<float>(wscale, N); g.N = N; g.K = K;
  const bf16_t* dX = r.in<bf16_t>(hx.data(), hx.size());
  uint8_t* dX8 = r.out<uint8_t>(x8_out, mx_x_bytes(K, G), "x8"); uint8_t* dXS = r.out<uint8_t>(xs_out, mx_s_bytes(K, G), "xs");
  float* dY = r.out<float>(mode == 2 ? nullptr : hy.data(), ny, "Y");
  g.bs = r.in<BatchState>(&hbs, 1);
  uint8_t* dY8 = r.out<uint8_t>(mode == 2 ? y8_out : nullptr, mx_x_bytes(ff, 16), "y8");
  uint8_t* dYS = r.out<uint8_t>(mode == 2 ? ys_out : nullptr, mx_s_bytes(ff, 16), "ys");
  g.X8 = dX8; g.XS = dXS; g.nt = nslots / 16; g.logits = dY; g.kpart = dY;
  g.d = K; g.ff = ff; g.H = 1; g.KVH = 1; g.Y8 = dY8; g.YS = dYS;
  if (const int rc = r.upload(s)) return rc;
  HIPCHK(c, hipMemsetAsync(dY, 0, ny * 4, s));
  HIPCHK(c, hipMemsetAsync(dY8, 0, mx_x_bytes(ff, 16), s));
  HIPCHK(c, hipMemsetAsync(dYS, 0, mx_s_bytes(ff, 16), s));
  launch_retile_mx(dW, dWm, N, K, G, s);
  launch_quant_mx_rows(dX, K, dX8, dXS, G, 64, s);
  if (mode == 0) launch_gemv_mxu(EPI_LOGITS, g, s);
  else if (mode == 2) launch_gemv_mxu(EPI_SWIGLU, g, s);
  else if (!launch_gemv_mxk(g, G, s)) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_mx: no K-slice kernel for N %d K %d G %d", N, K, G);
  if (const int rc = r.finish(s)) return rc;
  if (mode == 0) memcpy(Y, hy.data(), (size_t)nslots * N * 4);
  else if (mode == 1)
    for (int sl = 0; sl < nslots; ++sl)
      for (int n = 0; n < N; ++n) {
        float sum = 0.f;
        for (int ks = 0; ks < 8; ++ks) sum += hy[((size_t)ks * 64 + sl) * N + n];
        Y[(size_t)sl * N + n] = sum;
      }
  return DTK_OK;
}

int dtk_op_attention(dtk_ctx* c, const uint16_t* Q, const uint16_t* K, const uint16_t* V, int H, int Tq, int Tk, int hd, int causal, int q_offset, uint16_t* O) {
  if (!c || !Q || !K || !V || !O) return fail(c, DTK_ERR_ARG, "dtk_op_attention: null argument");
  if (hd != 72 && hd != 128 && hd != 64 && hd != 32) return fail(c, DTK_ERR_ARG, "unsupported head dim %d", hd);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, "dtk_op_attention");
  AttnArgs a;
  a.Q = r.in<bf16_t>(Q, (size_t)H * Tq * hd); a.q_sh = (long)Tq * hd; a.q_st = hd;
  a.K = r.in<bf16_t>(K, (size_t)H * Tk * hd); a.k_sh = (long)Tk * hd; a.k_st = hd;
  a.V = r.in<bf16_t>(V, (size_t)H * Tk * hd); a.v_sh = (long)Tk * hd; a.v_st = hd;
  a.O = r.out<bf16_t>(O, (size_t)H * Tq * hd, "O"); a.o_sh = (long)Tq * hd; a.o_st = hd;
  a.H = H; a.Tq = Tq; a.Tk = Tk; a.hd = hd; a.causal = causal; a.q_offset = q_offset;
  a.scale = 1.0f / sqrtf((float)hd); a.impl = c->attn_impl; a.kv_group = 1;
  if (const int rc = r.upload(s)) return rc;
  launch_attention(a, s);
  return r.finish(s);
}

int dtk_op_attention_seg(dtk_ctx* c, const uint16_t* Q, const uint16_t* K, const uint16_t* V, int H, int Tq, int Tk, int hd, int shared_len,
                         const int32_t* seg_begin, const int32_t* kv_row, uint16_t* O) {
  if (!c || !Q || !K || !V || !O || !seg_begin || !kv_row) return fail(c, DTK_ERR_ARG, "dtk_op_attention_seg: null argument");
  if (hd != 128 && hd != 64) return fail(c, DTK_ERR_ARG, "dtk_op_attention_seg: head dim %d (128 or 64)", hd);
  if (H < 1 || Tq < 1 || Tk < 1 || shared_len < 0 || shared_len > Tk) return fail(c, DTK_ERR_ARG, "dtk_op_attention_seg: bad shape");
  if (c->attn_impl == 1) return fail(c, DTK_ERR_STATE, "dtk_op_attention_seg: attn_impl = 1 (the VALU attention kernel) has no segmented form");
  std::vector<int32_t> rows((size_t)2 * Tq);
  for (int t = 0; t < Tq; ++t) {
    if (kv_row[t] < 0 || kv_row[t] >= Tk || seg_begin[t] < 0 || seg_begin[t] > kv_row[t])
      return fail(c, DTK_ERR_ARG, "dtk_op_attention_seg: row %d: segment begin %d, cache row %d of %d keys", t, seg_begin[t], kv_row[t], Tk);
    rows[2 * (size_t)t] = seg_begin[t]; rows[2 * (size_t)t + 1] = kv_row[t];
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, "dtk_op_attention_seg");
  AttnArgs a;
  a.Q = r.in<bf16_t>(Q, (size_t)H * Tq * hd); a.q_sh = (long)Tq * hd; a.q_st = hd;
  a.K = r.in<bf16_t>(K, (size_t)H * Tk * hd); a.k_sh = (long)Tk * hd; a.k_st = hd;
  a.V = r.in<bf16_t>(V, (size_t)H * Tk * hd); a.v_sh = (long)Tk * hd; a.v_st = hd;
  a.O = r.out<bf16_t>(O, (size_t)H * Tq * hd, "O"); a.o_sh = (long)Tq * hd; a.o_st = hd;
  const int2* dR = r.in<int2>(rows.data(), (size_t)Tq);
  a.H = H; a.Tq = Tq; a.Tk = Tk; a.hd = hd; a.causal = 1; a.q_offset = 0;
  a.scale = 1.0f / sqrtf((float)hd); a.impl = c->attn_impl; a.kv_group = 1;
  if (const int rc = r.upload(s)) return rc;
  if (!launch_attention_seg(a, shared_len, dR, s)) return fail(c, DTK_ERR_ARG, "dtk_op_attention_seg: the kernel does not take these operands");
  return r.finish(s);
}

// The single-sequence decode attention alone (launch_attn_decode as decode_step_launches calls it) on host operands: q [H*hd], K / V
// [KVH][T_max][hd], scale hd^-0.5.  The caches are uploaded once; for each of the npos positions DecState.pos is set, the kernels of
// (threads, splits, mode) run and that position's head outputs go to out[i][H*hd].  mode = AttnDecArgs::combine: 2 own combine kernel,
// 1 in-kernel combine (threads 0; the arrival counters start at zero and must be zero again afterwards), 3 k_attn_decode_head (threads
// 0), 0 consumer-side combine: o_proj's PRO_ATTN / EPI_RESID GEMV with an identity [d][d] weight onto a zero residual (variant -1: the
// default of launch_gemv, 0..8: launch_gemv_variant), and the raw partials pm / pl [npos][H][S], po [npos][H][S][hd] come back too
// (NaN where the kernels wrote none: threads != 0 with one split writes the head output itself and o_proj copies it, as in the step).
int dtk_op_attn_decode(dtk_ctx* c, const uint16_t* q, const uint16_t* K, const uint16_t* V, int H, int KVH, int hd, int T_max,
                       const int32_t* pos, int npos, int threads, int splits, int mode, int variant, uint16_t* out,
                       float* pm_out, float* pl_out, float* po_out) {
  if (!c || !q || !K || !V || !pos || !out) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode: null argument");
  if (hd != 128 && hd != 64) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode: head dim %d (128 or 64)", hd);
  if (H < 1 || KVH < 1 || H % KVH || T_max < 1 || npos < 1 || npos > 4096) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode: bad shape");
  if (threads != 0 && threads != 256 && threads != 512 && threads != 1024) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode: threads must be 0, 256, 512 or 1024");
  if (threads == 0 && hd == 64) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode: threads 0 (contiguous splits) has no head_dim-64 kernel: 256, 512 or 1024");
  if (splits < 1 || splits > 16) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode: splits must be 1..16");
  if (mode < 0 || mode > 3) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode: mode must be 0..3");
  if ((mode == 1 || mode == 3) && threads != 0) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode: mode %d needs threads 0 (the tile kernel has no such form)", mode);
  if (variant < -1 || variant > 8) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode: variant must be -1 (default) or 0..8");
  if (mode == 0 && (!pm_out || !pl_out || !po_out)) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode: mode 0 returns the partials");
  for (int i = 0; i < npos; ++i)
    if (pos[i] < 0 || pos[i] >= T_max) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode: position %d of %d rows", pos[i], T_max);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int d = H * hd, S = splits;
  const size_t kv = (size_t)KVH * T_max * hd, part = (size_t)H * S * 130;   // 130: the in-kernel combine keeps (m, l) next to a split's 128 outputs
  const size_t hs = (size_t)npos * H * S;
  std::vector<DecState> hst((size_t)npos);
  memset(hst.data(), 0, sizeof(DecState) * (size_t)npos);
  for (int i = 0; i < npos; ++i) { hst[(size_t)i].pos = pos[i]; hst[(size_t)i].next_pos = pos[i] + 1; }
  std::vector<bf16_t> eye(mode == 0 ? (size_t)d * d : 0, (bf16_t)0);     // mode 0: o_proj's identity weight
  for (int i = 0; i < d && mode == 0; ++i) eye[(size_t)i * d + i] = 0x3F80;   // bf16 1.0
  std::vector<float> po(mode == 0 ? (size_t)npos * part : 0);
  std::vector<unsigned> ctr((size_t)H, 0u);
  OpRun r(c, "dtk_op_attn_decode");
  const bf16_t* dq = r.in<bf16_t>(q, d); const bf16_t* dK = r.in<bf16_t>(K, kv); const bf16_t* dV = r.in<bf16_t>(V, kv);
  const DecState* dst = r.in<DecState>(hst.data(), npos);
  float* dpm = r.out<float>(mode == 0 ? pm_out : nullptr, hs, "pm"); float* dpl = r.out<float>(mode == 0 ? pl_out : nullptr, hs, "pl");
  float* dpo = r.out<float>(mode == 0 ? po.data() : nullptr, (size_t)npos * part, "po");
  bf16_t* dout = r.out<bf16_t>(mode == 0 ? nullptr : out, (size_t)npos * d, "out");
  bf16_t* dy = r.out<bf16_t>(mode == 0 ? out : nullptr, (size_t)npos * d, "y");
  unsigned* dctr = r.out<unsigned>(ctr.data(), H, "counters");
  const bf16_t* dW = r.in<bf16_t>(mode == 0 ? eye.data() : nullptr, mode == 0 ? (size_t)d * d : 1);
  if (const int rc = r.upload(s)) return rc;
  if (mode == 0) HIPCHK(c, hipMemsetAsync(dy, 0, (size_t)npos * d * 2, s));       // the zero residual
  HIPCHK(c, hipMemsetAsync(dpm, 0xFF, hs * 4, s));
  HIPCHK(c, hipMemsetAsync(dpl, 0xFF, hs * 4, s));
  HIPCHK(c, hipMemsetAsync(dpo, 0xFF, (size_t)npos * part * 4, s));
  HIPCHK(c, hipMemsetAsync(dout, 0xFF, (size_t)npos * d * 2, s));
  HIPCHK(c, hipMemsetAsync(dctr, 0, (size_t)H * 4, s));
  for (int i = 0; i < npos; ++i) {
    AttnDecArgs ad;
    ad.q = dq; ad.kcache = dK; ad.vcache = dV; ad.st = dst + i;
    ad.pm = dpm + (size_t)i * H * S; ad.pl = dpl + (size_t)i * H * S; ad.po = dpo + (size_t)i * part;
    ad.H = H; ad.S = S; ad.T_max = T_max; ad.G = H / KVH; ad.scale = 1.0f / sqrtf((float)hd); ad.hd = hd;
    ad.threads = threads; ad.combine = mode; ad.out = dout + (size_t)i * d; ad.counters = dctr;
    launch_attn_decode(ad, s);
    if (mode != 0) continue;
    GemvArgs g{};
    g.W = dW; g.N = d; g.K = d; g.y = dy + (size_t)i * d; g.d = d; g.H = H; g.KVH = KVH; g.hd = hd; g.st = dst + i; g.T_max = T_max;
    g.pm = ad.pm; g.pl = ad.pl; g.po = ad.po; g.S = S;
    if (threads && S == 1) { g.x = ad.out; launch_gemv(PRO_COPY, EPI_RESID, g, s); }   // as decode_step_launches: no partials exist
    else if (variant < 0) launch_gemv(PRO_ATTN, EPI_RESID, g, s);
    else launch_gemv_variant(PRO_ATTN, EPI_RESID, variant, g, s);
  }
  if (const int rc = r.finish(s)) return rc;
  // [H][S][hd] of every position's [H][S][130] room
  for (int i = 0; i < npos && mode == 0; ++i) memcpy(po_out + (size_t)i * H * S * hd, po.data() + (size_t)i * part, (size_t)H * S * hd * 4);
  for (int h = 0; h < H; ++h)
    if (ctr[(size_t)h]) return fail(c, DTK_ERR_STATE, "dtk_op_attn_decode: arrival counter of head %d is %u after the launches (not zero)", h, ctr[(size_t)h]);
  return DTK_OK;
}

// The batched decode attention alone (launch_attn_decode_b as batch_step_launches / batch_step_launches_mv call it; bf16 output) on
// host operands: nslots = the grid's y (1, 2, 4: the multi-vector step, no prefix kernel; 16, 32, 64), q [nslots][H*128], K / V
// [nslots][KVH][T_max][128], per slot pos / active / share_src (-1: none) / share_len.  The prefix groups come from
// build_prefix_groups, the step's own table.  out [nslots][H*128] row-major (the fragment-major order of the kernel is undone here);
// every element is 0xFFFF first, so the rows of slots that did not decode keep that value.
//
// kv8_from != nullptr (dtk_op_attn_decode_b8): the KV8 instantiations on the caller's shadow planes — codes [nslots][KVH][T_max][128],
// scales [nslots][KVH][T_max][4], uploaded as they are (the caller's poison included) and read back after the launch.
static int op_attn_decode_b(dtk_ctx* c, const char* who, const uint16_t* q, const uint16_t* K, const uint16_t* V, int nslots, int H, int KVH, int T_max,
                            const int32_t* pos, const int32_t* active, const int32_t* share_src, const int32_t* share_len,
                            const int32_t* kv8_from, uint8_t* k8, uint8_t* k8s, uint8_t* v8, uint8_t* v8s,
                            int use_prefix, int pfx_splits, int tail_threads, int gqa_fused, int attn_nt, uint16_t* out) {
  if (!c || !q || !K || !V || !pos || !active || !share_src || !share_len || !out) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode_b: null argument");
  if (nslots != 1 && nslots != 2 && nslots != 4 && nslots != 16 && nslots != 32 && nslots != 64)
    return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode_b: nslots must be 1, 2, 4, 16, 32 or 64");
  if (H < 1 || KVH < 1 || H % KVH || T_max < 1) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode_b: bad shape");
  const int G = H / KVH;
  if (G != 1 && G != 2 && G != 4) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode_b: %d query heads per K/V head (1, 2 or 4)", G);
  if (pfx_splits < 1 || pfx_splits > 4) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode_b: pfx_splits must be 1..4");
  if (gqa_fused < 0 || gqa_fused > 2) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode_b: gqa_fused must be 0, 1 or 2");
  if (tail_threads != 64 && tail_threads != 128 && tail_threads != 256 && tail_threads != 512 && !(tail_threads == 1024 && nslots <= 4))
    return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode_b: tail_threads must be 64, 128, 256 or 512 (1024: the multi-vector step, nslots <= 4)");
  if (use_prefix && nslots < 16) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode_b: the multi-vector step has no prefix kernel");
  BatchState hbs; memset(&hbs, 0, sizeof hbs);
  int32_t act[DTK_MAX_BATCH] = {};
  for (int j = 0; j < DTK_MAX_BATCH; ++j) { hbs.share_src[j] = -1; hbs.share_len[j] = 0; }
  for (int j = 0; j < nslots; ++j) {
    if (pos[j] < 0 || pos[j] >= T_max) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode_b: slot %d: position %d of %d rows", j, pos[j], T_max);
    if (share_src[j] >= nslots || share_src[j] == j || (share_src[j] >= 0 && (share_len[j] < 0 || share_len[j] > pos[j])))
      return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode_b: slot %d: source %d, %d shared rows, position %d", j, share_src[j], share_len[j], pos[j]);
    act[j] = active[j] ? 1 : 0;
    hbs.active[j] = act[j];
    hbs.share_src[j] = share_src[j] >= 0 ? share_src[j] : -1;
    hbs.share_len[j] = share_src[j] >= 0 ? share_len[j] : 0;
    if (kv8_from) {
      if (act[j] && (kv8_from[j] < hbs.share_len[j] || kv8_from[j] > pos[j]))
        return fail(c, DTK_ERR_ARG, "%s: slot %d: kv8_from %d outside [%d shared rows, position %d]", who, j, kv8_from[j], hbs.share_len[j], pos[j]);
      hbs.kv8_from[j] = kv8_from[j];
    }
  }
  build_prefix_groups(&hbs, act, use_prefix != 0);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int d = H * 128, nsteps = (d + 31) >> 5;
  const size_t kv_slot = (size_t)KVH * T_max * 128, kv = (size_t)nslots * kv_slot;
  const size_t out_elems = (size_t)((nslots + 15) >> 4) * nsteps * 512, recs = (size_t)nslots * H * pfx_splits;
  std::vector<DecState> hst((size_t)nslots);
  memset(hst.data(), 0, sizeof(DecState) * (size_t)nslots);
  for (int j = 0; j < nslots; ++j) { hst[(size_t)j].pos = pos[j]; hst[(size_t)j].next_pos = pos[j] + 1; }
  std::vector<bf16_t> frag(out_elems);
  struct Big { void* p = nullptr; ~Big() { if (p) (void)hipFree(p); } } big;     // caches beyond the op scratch: allocated for this call
  OpRun r(c, "dtk_op_attn_decode_b");
  AttnDecBArgs ad;
  const size_t sh = kv8_from ? kv : 0;      // bytes of one shadow code plane (its scales: / 32)
  if (kv * 4 + sh * 2 + sh / 16 + ((size_t)8 << 20) > c->scratch_bytes) {
    HIPCHK(c, hipMalloc(&big.p, kv * 4 + sh * 2 + sh / 16));
    bf16_t* dK = (bf16_t*)big.p;
    ad.kcache = dK; ad.vcache = dK + kv;
    r.ins.push_back({dK, K, kv * 2}); r.ins.push_back({dK + kv, V, kv * 2});      // uploaded with the operands in the scratch
    if (kv8_from) {
      ad.k8 = (uint8_t*)(dK + 2 * kv); ad.v8 = ad.k8 + sh; ad.k8s = ad.v8 + sh; ad.v8s = ad.k8s + sh / 32;
      r.res.push_back({ad.k8, k8, sh, "k8", true}); r.res.push_back({ad.v8, v8, sh, "v8", true});
      r.res.push_back({ad.k8s, k8s, sh / 32, "k8s", true}); r.res.push_back({ad.v8s, v8s, sh / 32, "v8s", true});
    }
  } else {
    ad.kcache = r.in<bf16_t>(K, kv); ad.vcache = r.in<bf16_t>(V, kv);
    if (kv8_from) {
      ad.k8 = r.io<uint8_t>(k8, sh, "k8"); ad.v8 = r.io<uint8_t>(v8, sh, "v8");
      ad.k8s = r.io<uint8_t>(k8s, sh / 32, "k8s"); ad.v8s = r.io<uint8_t>(v8s, sh / 32, "v8s");
    }
  }
  ad.kv8_slot_stride = kv_slot;
  ad.q = r.in<bf16_t>(q, (size_t)nslots * d); ad.st = r.in<DecState>(hst.data(), nslots); ad.bs = r.in<BatchState>(&hbs, 1);
  ad.out = r.out<bf16_t>(frag.data(), out_elems, "out");
  ad.pfx_m = (float*)r.take(recs * 4); ad.pfx_l = (float*)r.take(recs * 4); ad.pfx_o = (float*)r.take(recs * 128 * 4);
  ad.kv_slot_stride = kv_slot; ad.H = H; ad.T_max = T_max; ad.d = d; ad.G = G; ad.nslots = nslots; ad.scale = 1.0f / sqrtf(128.f);
  ad.use_prefix = use_prefix != 0; ad.pfx_splits = pfx_splits; ad.tail_threads = tail_threads; ad.gqa_fused = gqa_fused; ad.nt_private = attn_nt != 0;
  if (const int rc = r.upload(s)) return rc;
  HIPCHK(c, hipMemsetAsync(ad.out, 0xFF, out_elems * 2, s));
  HIPCHK(c, hipMemsetAsync(ad.pfx_m, 0xFF, recs * 4, s));
  HIPCHK(c, hipMemsetAsync(ad.pfx_l, 0xFF, recs * 4, s));
  HIPCHK(c, hipMemsetAsync(ad.pfx_o, 0xFF, recs * 128 * 4, s));
  launch_attn_decode_b(ad, s);
  if (const int rc = r.finish(s)) return rc;
  if (kv8_from) {      // the bf16 caches are the master copy: the KV8 kernels read them and must leave every byte as it was uploaded
    std::vector<uint16_t> back(kv);
    for (int w = 0; w < 2; ++w) {
      HIPCHK(c, hipMemcpy(back.data(), w ? ad.vcache : ad.kcache, kv * 2, hipMemcpyDeviceToHost));
      const uint16_t* src = w ? V : K;
      if (memcmp(back.data(), src, kv * 2)) {
        size_t i = 0;
        while (back[i] == src[i]) ++i;
        return fail(c, DTK_ERR_STATE, "%s: bf16 %s element %zu (slot %zu, row %zu) changed during the launch: %#x -> %#x", who, w ? "V" : "K", i,
                    i / kv_slot, i % ((size_t)T_max * 128) / 128, (unsigned)src[i], (unsigned)back[i]);
      }
    }
  }
  for (int j = 0; j < nslots; ++j)
    for (int k = 0; k < d; ++k) out[(size_t)j * d + k] = frag[host_xtile_off(j, k, nsteps)];
  return DTK_OK;
}
int dtk_op_attn_decode_b(dtk_ctx* c, const uint16_t* q, const uint16_t* K, const uint16_t* V, int nslots, int H, int KVH, int T_max,
                         const int32_t* pos, const int32_t* active, const int32_t* share_src, const int32_t* share_len,
                         int use_prefix, int pfx_splits, int tail_threads, int gqa_fused, int attn_nt, uint16_t* out) {
  return op_attn_decode_b(c, "dtk_op_attn_decode_b", q, K, V, nslots, H, KVH, T_max, pos, active, share_src, share_len, nullptr, nullptr, nullptr,
                          nullptr, nullptr, use_prefix, pfx_splits, tail_threads, gqa_fused, attn_nt, out);
}
int dtk_op_attn_decode_b8(dtk_ctx* c, const uint16_t* q, const uint16_t* K, const uint16_t* V, int nslots, int H, int KVH, int T_max,
                          const int32_t* pos, const int32_t* active, const int32_t* share_src, const int32_t* share_len,
                          const int32_t* kv8_from, uint8_t* k8_codes, uint8_t* k8_scales, uint8_t* v8_codes, uint8_t* v8_scales,
                          int use_prefix, int pfx_splits, int tail_threads, int gqa_fused, int attn_nt, uint16_t* out) {
  if (!kv8_from || !k8_codes || !k8_scales || !v8_codes || !v8_scales) return fail(c, DTK_ERR_ARG, "dtk_op_attn_decode_b8: null argument");
  return op_attn_decode_b(c, "dtk_op_attn_decode_b8", q, K, V, nslots, H, KVH, T_max, pos, active, share_src, share_len, kv8_from, k8_codes,
                          k8_scales, v8_codes, v8_scales, use_prefix, pfx_splits, tail_threads, gqa_fused, attn_nt, out);
}

// ---- the single-sequence decode GEMV family alone (dtk_op_gemv_role): one (prologue, epilogue, weight format, shape) of k_gemv on
// host operands through the step's own launchers.  Everything the step would never hand these kernels is refused before anything is
// allocated, uploaded or launched.
static bool gemv_role_variant_ok(int fmt, int pro, int epi, int v) {     // fmt 0 bf16 (launch_gemv_variant), 1 fp8 (launch_gemv_f8_variant), 2 MXFP4 (launch_gemv_q4)
  if (fmt == 2) {
    const bool pair = (pro == PRO_RMSNORM && (epi == EPI_QKV || epi == EPI_SWIGLU || epi == EPI_STORE)) || (pro == PRO_ATTN && epi == EPI_RESID) ||
                      (pro == PRO_COPY && (epi == EPI_RESID || epi == EPI_STORE));
    return pair && v == -1;
  }
  if (fmt == 1) {
    const bool pair = (pro == PRO_RMSNORM && (epi == EPI_QKV || epi == EPI_SWIGLU || epi == EPI_LOGITS)) || ((pro == PRO_ATTN || pro == PRO_COPY) && epi == EPI_RESID);
    return pair && v >= -1 && v <= 9;
  }
  if (v < -1) return false;
  if (pro == PRO_RMSNORM && (epi == EPI_QKV || epi == EPI_SWIGLU)) return v <= 11;
  if (pro == PRO_COPY && epi == EPI_RESID) return v <= 22;
  if (pro == PRO_ATTN && epi == EPI_RESID) return v <= 8;
  if (pro == PRO_RMSNORM && epi == EPI_LOGITS) return v <= 4;
  if (pro == PRO_RMSNORM && epi == EPI_STORE) return v <= 0 || v == 20;
  if (pro == PRO_COPY && epi == EPI_STORE) return v <= 0 || v == 20 || v == 21;
  return false;
}

int dtk_op_gemv_role(dtk_ctx* c, int pro, int epi, int variant, const uint16_t* W, const uint8_t* W8, const float* wscale,
                     const uint8_t* W4, const uint8_t* S4, int N, int K, int d, int ff, int H, int KVH, int hd, int T_max, int pos, float eps,
                     const uint16_t* x, const uint16_t* norm_w, const uint16_t* rope_cos, const uint16_t* rope_sin,
                     int S, const float* pm, const float* pl, const float* po, int scratch_fill,
                     uint16_t* q_io, uint16_t* k_io, uint16_t* v_io, uint16_t* y_io, float* logits_io) {
  if (!c) return DTK_ERR_ARG;
  if ((W != nullptr) + (W8 != nullptr) + (W4 != nullptr) != 1 || (W8 && !wscale) || (!W8 && wscale) || (!W4 != !S4))
    return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: exactly one of W | W8 + wscale | W4 + S4");
  const int fmt = W4 ? 2 : (W8 ? 1 : 0);
  // variant 0x1000 + v on bf16 operands: W is packed into 13-bit planes on the device (launch_pack_w13_rows) and the role streams those in
  // 13-bit shape v (0xff: the shape a decode step runs); with an unpackable row the planes are dropped and launch_gemv takes the bf16 kernel
  const bool f13 = variant >= 0x1000;
  const int v13 = variant - 0x1000;
  if (f13) {
    if (fmt != 0) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: the 13-bit planes are packed from bf16 operands (W)");
    if (v13 != 0xff && !gemv_w13_has(pro, epi, v13)) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: no 13-bit kernel for prologue %d, epilogue %d, shape %d", pro, epi, v13);
    if (v13 == 0xff && !gemv_w13_has(pro, epi, 0)) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: no 13-bit kernel for prologue %d, epilogue %d", pro, epi);
    variant = -1;
  }
  if (N < 1 || K < 8 || (K & 7) || (fmt == 1 && (K & 15))) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: N >= 1, K a multiple of 8 (16 for fp8 weights)");
  if (pro < PRO_COPY || pro > PRO_ATTN || epi < EPI_STORE || epi > EPI_LOGITS) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: unknown prologue %d or epilogue %d", pro, epi);
  if (!gemv_role_variant_ok(fmt, pro, epi, variant))
    return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: no %s kernel for prologue %d, epilogue %d, variant %d", fmt == 2 ? "MXFP4" : (fmt == 1 ? "fp8" : "bf16"), pro, epi, variant);
  if (hd != 128 && hd != 64) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: head dim %d (128 or 64)", hd);
  if (scratch_fill < 0 || scratch_fill > 255 || d < 0) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: scratch_fill is a byte, d >= 0");
  if (pro == PRO_ATTN) {
    if (S < 1 || S > 16) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: S must be 1..16");
    if (H < 1 || K != H * hd || !pm || !pl || !po) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: PRO_ATTN needs K = H * hd and the partials pm / pl / po");
  } else if (!x || (pro == PRO_RMSNORM && !norm_w)) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: x (and norm_w for PRO_RMSNORM) required");
  if (epi == EPI_QKV) {
    if (H < 1 || KVH < 1 || H % KVH) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: H %d query heads over KVH %d key / value heads", H, KVH);
    if (N != (H + 2 * KVH) * hd || d != H * hd) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: QKV needs N = (H + 2 KVH) * hd and d = H * hd");
    if (T_max < 1 || pos < 0 || pos >= T_max) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: position %d of %d rows", pos, T_max);
    if (!rope_cos || !rope_sin || !q_io || !k_io || !v_io) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: QKV needs the rope tables and q / k / v buffers");
  } else if (epi == EPI_SWIGLU) {
    if (ff < 8 || (ff & 7) || N != 2 * ff || !y_io) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: SWIGLU needs ff a multiple of 8 (as dtk_create), N = 2 ff and y");
  } else if (epi == EPI_LOGITS) {
    if (!logits_io) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: LOGITS needs the logits buffer");
  } else if (!y_io) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_role: RESID / STORE need y");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int KC4 = (K + 31) >> 5, hd2 = hd / 2;
  const size_t w_bytes = fmt == 2 ? (size_t)N * KC4 * 16 : (fmt == 1 ? (size_t)N * K : (size_t)N * K * 2);
  const size_t kv = epi == EPI_QKV ? (size_t)KVH * T_max * hd : 0, qn = epi == EPI_QKV ? (size_t)H * hd : 0, rope = epi == EPI_QKV ? (size_t)T_max * hd2 : 0;
  const size_t ny = epi == EPI_SWIGLU ? (size_t)ff : ((epi == EPI_STORE || epi == EPI_RESID) ? (size_t)N : 0), nl = epi == EPI_LOGITS ? (size_t)N : 0;
  const size_t hs = pro == PRO_ATTN ? (size_t)H * S : 0;
  DecState hst; memset(&hst, 0, sizeof hst);
  hst.pos = pos; hst.next_pos = pos + 1;
  OpRun r(c, "dtk_op_gemv_role", scratch_fill);
  GemvArgs g{};
  const uint8_t* dW = r.in<uint8_t>(fmt == 2 ? (const void*)W4 : (fmt == 1 ? (const void*)W8 : (const void*)W), w_bytes);
  const float* dws = r.in<float>(wscale, fmt == 1 ? N : 0); const uint8_t* dS4 = r.in<uint8_t>(S4, fmt == 2 ? (size_t)N * KC4 : 0);
  if (fmt == 0) g.W = reinterpret_cast<const bf16_t*>(dW);
  else if (fmt == 1) { g.W8 = dW; g.wscale = dws; }
  else { g.W4 = dW; g.S4 = dS4; }
  uint8_t* dWp = (uint8_t*)r.take(f13 ? (size_t)N * w13_row_bytes(K) : 0); uint8_t* dWh = (uint8_t*)r.take(f13 ? (size_t)N : 0);
  unsigned* dbad = (unsigned*)r.take(f13 ? sizeof(unsigned) : 0);
  g.x = r.in<bf16_t>(pro != PRO_ATTN ? x : nullptr, K); g.norm_w = r.in<bf16_t>(pro == PRO_RMSNORM ? norm_w : nullptr, K);
  g.rope_cos = r.in<bf16_t>(rope_cos, rope); g.rope_sin = r.in<bf16_t>(rope_sin, rope); g.st = r.in<DecState>(&hst, 1);
  g.pm = r.in<float>(pm, hs); g.pl = r.in<float>(pl, hs); g.po = r.in<float>(po, hs * hd);
  // a role writes its own cells only: nothing behind the end of q / k / v / y / logits
  g.q_out = r.io<bf16_t>(qn ? q_io : nullptr, qn, "q"); g.kcache = r.io<bf16_t>(kv ? k_io : nullptr, kv, "k"); g.vcache = r.io<bf16_t>(kv ? v_io : nullptr, kv, "v");
  g.y = r.io<bf16_t>(ny ? y_io : nullptr, ny, "y"); g.logits = r.io<float>(nl ? logits_io : nullptr, nl, "logits");
  g.N = N; g.K = K; g.eps = eps; g.S = S; g.T_max = T_max; g.d = d; g.ff = ff; g.H = H; g.KVH = KVH; g.hd = hd;
  if (const int rc = r.upload(s)) return rc;      // (hst lives on this frame)
  if (f13) {
    unsigned bad = 0;
    HIPCHK(c, hipMemsetAsync(dbad, 0, sizeof(unsigned), s));
    launch_pack_w13_rows(g.W, dWp, dWh, dbad, N, K, !c->w13_nz, s);
    HIPCHK(c, hipMemcpyAsync(&bad, dbad, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipMemsetAsync(dbad, scratch_fill, sizeof(unsigned), s));
    c->w13_op_bad_rows = (int)bad;
    if (!bad) { g.Wp = dWp; g.Wh = dWh; }
  }
  if (f13 && g.Wp && v13 != 0xff) launch_gemv_w13_variant(pro, epi, v13, g, s);
  else if (variant < 0) launch_gemv(pro, epi, g, s);
  else if (fmt == 1) launch_gemv_f8_variant(pro, epi, variant, g, s);
  else launch_gemv_variant(pro, epi, variant, g, s);
  return r.finish(s);
}

// ---- the prefill's row kernels and attention layouts alone (dtk_op_rope_scatter / _rows_norm / _swiglu / _attention_ex / _rows_move):
// host operands into the op scratch as dtk_op_gemv_role does it — the whole scratch the op uses is filled with scratch_fill first, every
// result buffer is in/out with 256 guard bytes behind it that must still hold scratch_fill after the launch, and everything the prefill
// would never hand a kernel is refused before anything is uploaded.

int dtk_op_rope_scatter(dtk_ctx* c, int form, const uint16_t* QKV, const float* part, int S, int part_rows, int T, int H, int KVH, int hd,
                        int T_max, int start_pos, const int32_t* rows, int max_pos, const uint16_t* rope_cos, const uint16_t* rope_sin,
                        int scratch_fill, uint16_t* q_io, uint16_t* k_io, uint16_t* v_io) {
  const char* who = "dtk_op_rope_scatter";
  if (!c || !rope_cos || !rope_sin || !q_io || !k_io || !v_io) return fail(c, DTK_ERR_ARG, "%s: null argument", who);
  if (form != 0 && form != 1) return fail(c, DTK_ERR_ARG, "%s: form %d (0 bf16 rows, 1 fp32 K-slice partials)", who, form);
  if (hd != 128 && hd != 64) return fail(c, DTK_ERR_ARG, "%s: head dim %d (128 or 64)", who, hd);
  if (T < 1 || H < 1 || KVH < 1 || H % KVH || T_max < 1 || max_pos < 1) return fail(c, DTK_ERR_ARG, "%s: T %d, H %d query heads over KVH %d key / value heads, T_max %d", who, T, H, KVH, T_max);
  if (scratch_fill < 0 || scratch_fill > 255) return fail(c, DTK_ERR_ARG, "%s: scratch_fill is a byte", who);
  if (form == 0 && !QKV) return fail(c, DTK_ERR_ARG, "%s: form 0 needs QKV", who);
  if (form == 1 && (!part || S < 1 || S > 8 || part_rows < T)) return fail(c, DTK_ERR_ARG, "%s: form 1 needs partials of S = 1..8 slices and part_rows >= T", who);
  for (int t = 0; t < T; ++t) {
    const int pos = rows ? rows[2 * t] : start_pos + t, row = rows ? rows[2 * t + 1] : start_pos + t;
    if (pos < 0 || pos >= max_pos || row < 0 || row >= T_max)
      return fail(c, DTK_ERR_ARG, "%s: row %d: position %d of %d, cache row %d of %d", who, t, pos, max_pos, row, T_max);
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t qkvn = (size_t)(H + 2 * KVH) * hd, kv = (size_t)KVH * T_max * hd;
  OpRun r(c, who, scratch_fill);
  const bf16_t* dQKV = r.in<bf16_t>(form == 0 ? QKV : nullptr, form == 0 ? (size_t)T * qkvn : 0);
  const float* dP = r.in<float>(form == 1 ? part : nullptr, form == 1 ? (size_t)S * part_rows * qkvn : 0);
  const bf16_t* dcos = r.in<bf16_t>(rope_cos, (size_t)max_pos * (hd / 2));
  const bf16_t* dsin = r.in<bf16_t>(rope_sin, (size_t)max_pos * (hd / 2));
  const int2* dR = r.in<int2>(rows, rows ? (size_t)T : 0);
  bf16_t* dq = r.io<bf16_t>(q_io, (size_t)H * T * hd, "q"); bf16_t* dk = r.io<bf16_t>(k_io, kv, "k"); bf16_t* dv = r.io<bf16_t>(v_io, kv, "v");
  if (const int rc = r.upload(s)) return rc;
  const long ps = (long)part_rows * (long)qkvn;
  if (form == 0 && rows) launch_rope_scatter_rows(dQKV, dq, dk, dv, dcos, dsin, T, dR, H, KVH, T_max, s, hd);
  else if (form == 0) launch_rope_scatter(dQKV, dq, dk, dv, dcos, dsin, T, start_pos, H, KVH, T_max, s, hd);
  else if (rows) launch_sk_rope_scatter_rows(dP, ps, S, dq, dk, dv, dcos, dsin, T, dR, H, KVH, T_max, s, hd);
  else launch_sk_rope_scatter(dP, ps, S, dq, dk, dv, dcos, dsin, T, start_pos, H, KVH, T_max, s, hd);
  return r.finish(s);
}

int dtk_op_rows_norm(dtk_ctx* c, int form, const uint16_t* X, const float* part, int S, int part_rows, const uint16_t* norm_w,
                     const uint16_t* ln_b, const uint16_t* bias, const uint16_t* residual, const uint16_t* gate, int flags, int M, int N,
                     int ldx, int ldc, int ldr, int ldy, float eps, int scratch_fill, uint16_t* c_io, uint16_t* y_io) {
  const char* who = "dtk_op_rows_norm";
  if (!c) return DTK_ERR_ARG;
  if (form < 0 || form > 3) return fail(c, DTK_ERR_ARG, "%s: form %d (0 rmsnorm_rows, 1 rmsnorm_rows_sk, 2 sk_reduce, 3 layernorm_rows)", who, form);
  if (M < 1 || N < 1 || scratch_fill < 0 || scratch_fill > 255) return fail(c, DTK_ERR_ARG, "%s: M, N >= 1, scratch_fill a byte", who);
  const bool in_place = form == 3 && !X;              // Y == X (the cross layer's q_norm)
  if (form != 2) {
    if (!y_io || !norm_w || (!X && !in_place) || (form == 3 && !ln_b)) return fail(c, DTK_ERR_ARG, "%s: null argument", who);
    if (in_place) ldx = ldy;
    if (ldx < N || ldy < N) return fail(c, DTK_ERR_ARG, "%s: ldx %d / ldy %d below the row length %d", who, ldx, ldy, N);
    if ((form == 0 || form == 3) && ((N % 8) || (ldx % 8) || (ldy % 8))) return fail(c, DTK_ERR_ARG, "%s: form %d reads and writes 16-byte chunks: D, ldx, ldy multiples of 8", who, form);
    if (form == 1 && (N % 4)) return fail(c, DTK_ERR_ARG, "%s: form 1 needs N %% 4 == 0", who);
  } else {
    const int known = DTK_EPI_BIAS | DTK_EPI_RESIDUAL | DTK_EPI_GATED_RESIDUAL;
    if (!part || !c_io || (norm_w && !y_io) || (flags & ~known)) return fail(c, DTK_ERR_ARG, "%s: form 2 needs partials and C (and Y with norm_w); flags: bias, residual, gated residual", who);
    if ((N % 4) || S < 1 || S > 8 || part_rows < M) return fail(c, DTK_ERR_ARG, "%s: form 2 needs N %% 4 == 0, S = 1..8 and part_rows >= M", who);
    if (((flags & DTK_EPI_BIAS) && !bias) || ((flags & DTK_EPI_RESIDUAL) && (!residual || ldr < N)) ||
        ((flags & DTK_EPI_GATED_RESIDUAL) && (!gate || !(flags & DTK_EPI_RESIDUAL))))
      return fail(c, DTK_ERR_ARG, "%s: a flag without its operand (the gated residual needs the residual too)", who);
    if (ldc < N || (norm_w && ldy < N)) return fail(c, DTK_ERR_ARG, "%s: ldc / ldy below N", who);
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, who, scratch_fill);
  if (form != 2) {
    const bf16_t* dX = in_place ? nullptr : r.in<bf16_t>(X, (size_t)M * ldx);
    const bf16_t* dw = r.in<bf16_t>(norm_w, N);
    const bf16_t* db = r.in<bf16_t>(form == 3 ? ln_b : nullptr, form == 3 ? N : 0);
    bf16_t* dY = r.io<bf16_t>(y_io, (size_t)M * ldy, "y");
    if (in_place) dX = dY;
    if (const int rc = r.upload(s)) return rc;
    if (form == 0) launch_rmsnorm_rows(dX, ldx, dw, dY, ldy, M, N, eps, s);
    else if (form == 1) launch_rmsnorm_rows_sk(dX, ldx, dw, dY, ldy, M, N, eps, s);
    else launch_layernorm_rows(dX, ldx, dw, db, dY, ldy, M, N, eps, s);
    return r.finish(s);
  }
  GemmArgs g;
  g.A = nullptr; g.lda = 0; g.W = nullptr; g.ldw = 0; g.M = M; g.N = N; g.K = 0; g.kslices = S;
  g.part = r.in<float>(part, (size_t)S * part_rows * N); g.part_stride = (long)part_rows * N;
  g.bias = r.in<bf16_t>((flags & DTK_EPI_BIAS) ? bias : nullptr, (flags & DTK_EPI_BIAS) ? N : 0);
  g.residual = r.in<bf16_t>((flags & DTK_EPI_RESIDUAL) ? residual : nullptr, (flags & DTK_EPI_RESIDUAL) ? (size_t)M * ldr : 0); g.ldr = ldr;
  g.gate = r.in<bf16_t>((flags & DTK_EPI_GATED_RESIDUAL) ? gate : nullptr, (flags & DTK_EPI_GATED_RESIDUAL) ? 1 : 0);
  const bf16_t* dw = r.in<bf16_t>(norm_w, norm_w ? N : 0);
  g.C = r.io<bf16_t>(c_io, (size_t)M * ldc, "c"); g.ldc = ldc;
  bf16_t* dY = r.io<bf16_t>(norm_w ? y_io : nullptr, norm_w ? (size_t)M * ldy : 0, "y");
  g.flags = ((flags & DTK_EPI_BIAS) ? GEMM_BIAS : 0) | ((flags & DTK_EPI_RESIDUAL) ? GEMM_RESIDUAL : 0) | ((flags & DTK_EPI_GATED_RESIDUAL) ? GEMM_GATED_RESIDUAL : 0);
  if (const int rc = r.upload(s)) return rc;
  launch_sk_reduce(g, norm_w ? dw : nullptr, dY, ldy, eps, s);
  return r.finish(s);
}

int dtk_op_swiglu(dtk_ctx* c, int form, const uint16_t* GU, const float* part, int S, int part_rows, const uint16_t* A, const uint16_t* W,
                  int M, int ff, int K, int ldact, int scratch_fill, uint16_t* act_io) {
  const char* who = "dtk_op_swiglu";
  if (!c) return DTK_ERR_ARG;
  if (form < 0 || form > 2) return fail(c, DTK_ERR_ARG, "%s: form %d (0 silu_mul, 1 sk_reduce_swiglu, 2 the GEMM epilogue)", who, form);
  if (!act_io || M < 1 || ff < 1 || ldact < ff || scratch_fill < 0 || scratch_fill > 255) return fail(c, DTK_ERR_ARG, "%s: act, M, ff >= 1, ldact >= ff, scratch_fill a byte", who);
  if (form == 0 && (!GU || (ff % 8) || ldact != ff)) return fail(c, DTK_ERR_ARG, "%s: form 0 needs GU, ff %% 8 == 0 (as dtk_create) and ldact == ff", who);
  if (form == 1 && (!part || S < 1 || S > 8 || (ff % 4) || (ldact % 4) || part_rows < M)) return fail(c, DTK_ERR_ARG, "%s: form 1 needs partials of S = 1..8 slices, ff %% 4 == 0, ldact %% 4 == 0, part_rows >= M", who);
  if (form == 2 && (!A || !W || K < 8 || (K % 8))) return fail(c, DTK_ERR_ARG, "%s: form 2 needs A, W and K %% 8 == 0", who);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, who, scratch_fill);
  if (form == 0) {
    const bf16_t* dGU = r.in<bf16_t>(GU, (size_t)M * 2 * ff);
    bf16_t* dA = r.io<bf16_t>(act_io, (size_t)M * ff, "act");
    if (const int rc = r.upload(s)) return rc;
    launch_silu_mul(dGU, ff, dA, M, s);
    return r.finish(s);
  }
  GemmArgs g;
  g.M = M; g.N = 2 * ff; g.K = K; g.flags = 0; g.bias = nullptr; g.residual = nullptr; g.ldr = 0;
  if (form == 1) {
    g.A = nullptr; g.lda = 0; g.W = nullptr; g.ldw = 0; g.C = nullptr; g.ldc = 0; g.kslices = S;
    g.part = r.in<float>(part, (size_t)S * part_rows * 2 * ff); g.part_stride = (long)part_rows * 2 * ff;
    bf16_t* dA = r.io<bf16_t>(act_io, (size_t)M * ldact, "act");
    if (const int rc = r.upload(s)) return rc;
    launch_sk_reduce_swiglu(g, dA, ldact, s);
    return r.finish(s);
  }
  g.A = r.in<bf16_t>(A, (size_t)M * K); g.lda = K;
  g.W = r.in<bf16_t>(W, (size_t)2 * ff * K); g.ldw = K;
  bf16_t* dWt = (bf16_t*)r.take(tiled_elems(2 * ff, K) * sizeof(bf16_t));
  g.Wt = dWt;
  g.C = r.io<bf16_t>(act_io, (size_t)M * ldact, "act"); g.ldc = ldact;
  if (r.full) return fail(c, DTK_ERR_ARG, "%s: op scratch exhausted", who);
  // the launcher's own refusals, asked before anything is uploaded: a dry call is not possible (it launches), so its conditions are restated
  if (K < 128 || ((2 * ff) & 31) || (ldact & 3)) return fail(c, DTK_ERR_ARG, "%s: k_gemm_g3's SwiGLU epilogue needs K >= 128, ff %% 16 == 0 and ldact %% 4 == 0", who);
  if (const int rc = r.upload(s)) return rc;
  launch_retile_pairs(g.W, dWt, ff, K, s);
  if (!launch_gemm_g3_swiglu(g, s)) {
    (void)hipStreamSynchronize(s);
    return fail(c, DTK_ERR_ARG, "%s: launch_gemm_g3_swiglu does not take this shape (\"gemm_g3_min_blocks\", \"gemm_wt\")", who);
  }
  return r.finish(s);
}

int dtk_op_attention_ex(dtk_ctx* c, const uint16_t* Q, int64_t nq, const uint16_t* K, int64_t nk, const uint16_t* V, int64_t nv,
                        uint16_t* o_io, int64_t no, const int64_t* strides, int H, int kv_group, int Tq, int Tk, int hd, int causal,
                        int q_offset, int nbatch, int scratch_fill) {
  const char* who = "dtk_op_attention_ex";
  if (!c || !Q || !K || !V || !o_io || !strides) return fail(c, DTK_ERR_ARG, "%s: null argument", who);
  if (hd != 72 && hd != 128 && hd != 64 && hd != 32) return fail(c, DTK_ERR_ARG, "%s: unsupported head dim %d", who, hd);
  if (H < 1 || Tq < 1 || Tk < 1 || nbatch < 1 || kv_group < 1 || H % kv_group || q_offset < 0 || scratch_fill < 0 || scratch_fill > 255)
    return fail(c, DTK_ERR_ARG, "%s: bad shape (H %d, kv_group %d, Tq %d, Tk %d, nbatch %d, q_offset %d)", who, H, kv_group, Tq, Tk, nbatch, q_offset);
  // strides = {q_sh, q_st, q_sb, k_sh, k_st, k_sb, v_sh, v_st, v_sb, o_sh, o_st, o_sb}, in elements
  const int64_t n[4] = {nq, nk, nv, no};
  const int heads[4] = {H, H / kv_group, H / kv_group, H}, toks[4] = {Tq, Tk, Tk, Tq};
  for (int i = 0; i < 4; ++i) {
    const int64_t sh = strides[3 * i], st = strides[3 * i + 1], sb = strides[3 * i + 2];
    if (sh < 0 || st < 0 || sb < 0 || n[i] < 1 || (sh | st | sb) >> 40) return fail(c, DTK_ERR_ARG, "%s: negative or absurd stride / size of operand %d", who, i);
    const int64_t last = (int64_t)(nbatch - 1) * sb + (int64_t)(heads[i] - 1) * sh + (int64_t)(toks[i] - 1) * st + hd;
    if (last > n[i]) return fail(c, DTK_ERR_ARG, "%s: the strides of %s address element %lld of %lld", who, i == 0 ? "Q" : (i == 1 ? "K" : (i == 2 ? "V" : "O")), (long long)last, (long long)n[i]);
    if ((sh | st | sb) & 1) return fail(c, DTK_ERR_ARG, "%s: odd stride (the kernels read and write bf16 pairs)", who);
  }
  AttnArgs a;
  a.q_sh = (long)strides[0]; a.q_st = (long)strides[1]; a.q_sb = (long)strides[2];
  a.k_sh = (long)strides[3]; a.k_st = (long)strides[4]; a.k_sb = (long)strides[5];
  a.v_sh = (long)strides[6]; a.v_st = (long)strides[7]; a.v_sb = (long)strides[8];
  a.o_sh = (long)strides[9]; a.o_st = (long)strides[10]; a.o_sb = (long)strides[11];
  a.H = H; a.Tq = Tq; a.Tk = Tk; a.hd = hd; a.causal = causal ? 1 : 0; a.q_offset = q_offset;
  a.scale = 1.0f / sqrtf((float)hd); a.impl = c->attn_impl; a.kv_group = kv_group; a.nbatch = nbatch;
  if (c->attn_impl == 2 && (!attention_mfma_operands(a) || (a.q_sb % 8) || (a.k_sb % 8) || (a.v_sb % 8) || (a.o_sb % 4)))
    return fail(c, DTK_ERR_ARG, "%s: attn_impl = 2 and the MFMA kernel does not take these operands (hd 128 / 72 / 64, Q / K / V strides %% 8, O strides %% 4)", who);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, who, scratch_fill);
  a.Q = r.in<bf16_t>(Q, (size_t)nq); a.K = r.in<bf16_t>(K, (size_t)nk); a.V = r.in<bf16_t>(V, (size_t)nv);
  a.O = r.io<bf16_t>(o_io, (size_t)no, "o");
  if (const int rc = r.upload(s)) return rc;
  launch_attention(a, s);
  return r.finish(s);
}

int dtk_op_rows_move(dtk_ctx* c, int form, const int32_t* ids, const uint16_t* src, const float* pixels, int M, int D, int V, int lds,
                     int ldd, int image, int patch, int scratch_fill, uint16_t* dst_io) {
  const char* who = "dtk_op_rows_move";
  if (!c) return DTK_ERR_ARG;
  if (form < 0 || form > 2) return fail(c, DTK_ERR_ARG, "%s: form %d (0 embed_gather, 1 copy_rows, 2 im2col)", who, form);
  if (!dst_io || scratch_fill < 0 || scratch_fill > 255) return fail(c, DTK_ERR_ARG, "%s: dst, scratch_fill a byte", who);
  if (form == 0) {
    if (!ids || !src || M < 1 || V < 1 || D < 8 || (D % 8)) return fail(c, DTK_ERR_ARG, "%s: form 0 needs ids, the table, d %% 8 == 0", who);
    for (int t = 0; t < M; ++t) if (ids[t] < 0 || ids[t] >= V) return fail(c, DTK_ERR_ARG, "%s: id %d of row %d outside [0, %d)", who, ids[t], t, V);
  } else if (form == 1) {
    if (!src || M < 1 || D < 8 || (D % 8) || lds < D || ldd < D || (lds % 8) || (ldd % 8)) return fail(c, DTK_ERR_ARG, "%s: form 1 needs src, D, lds, ldd multiples of 8, lds / ldd >= D", who);
  } else if (!pixels || patch < 1 || image < patch || ldd < 3 * patch * patch) return fail(c, DTK_ERR_ARG, "%s: form 2 needs pixels, image >= patch >= 1, ldp >= 3 patch^2", who);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, who, scratch_fill);
  if (form == 0) {
    const int32_t* di = r.in<int32_t>(ids, M); const bf16_t* de = r.in<bf16_t>(src, (size_t)V * D);
    bf16_t* dX = r.io<bf16_t>(dst_io, (size_t)M * D, "x");
    if (const int rc = r.upload(s)) return rc;
    launch_embed_gather(di, de, dX, M, D, s);
  } else if (form == 1) {
    const bf16_t* ds = r.in<bf16_t>(src, (size_t)M * lds);
    bf16_t* dd = r.io<bf16_t>(dst_io, (size_t)M * ldd, "dst");
    if (const int rc = r.upload(s)) return rc;
    launch_copy_rows(ds, lds, dd, ldd, M, D, s);
  } else {
    const int np = image / patch;
    const float* dp = r.in<float>(pixels, (size_t)3 * image * image);
    bf16_t* dd = r.io<bf16_t>(dst_io, (size_t)np * np * ldd, "patches");
    if (const int rc = r.upload(s)) return rc;
    launch_im2col(dp, dd, image, patch, ldd, s);
  }
  return r.finish(s);
}

// ---- the multi-vector decode GEMV family alone (dtk_op_gemv_mv_role): one (prologue, epilogue) of k_gemv_mv on host operands through
// the step's own launcher, nb = 1 | 2 | 4 slots with their own positions and active flags.  Fragment-order buffers (x_layout 1, the SwiGLU
// activation) cross the ABI as the kernel holds them, whole 16-slot tiles.  The block shape is set for this call alone.
extern "C++" {
namespace {
struct MvShapeScope {      // launch_gemv_mv reads the shape table: o_proj (K == d) looks at role 5 first
  int epi;
  MvShapeScope(int epi_, int shape) : epi(epi_) { set_gemv_mv_shape(epi, shape); if (epi == EPI_RESID) set_gemv_mv_shape(5, shape); }
  ~MvShapeScope() { set_gemv_mv_shape(epi, -1); if (epi == EPI_RESID) set_gemv_mv_shape(5, -1); }
};
}  // namespace
}  // extern "C++"

int dtk_op_gemv_mv_role(dtk_ctx* c, int pro, int epi, int nb, int shape, const uint16_t* W, const uint8_t* W8, const float* wscale,
                        int N, int K, int d, int ff, int H, int KVH, int T_max, const int32_t* pos, const int32_t* active, int bs_null,
                        int x_layout, const uint16_t* X, const uint16_t* norm_w, float eps, const uint16_t* rope_cos,
                        const uint16_t* rope_sin, int scratch_fill, uint16_t* q_io, uint16_t* k_io, uint16_t* v_io, uint16_t* y_io,
                        float* logits_io) {
  const char* who = "dtk_op_gemv_mv_role";
  if (!c) return DTK_ERR_ARG;
  if ((W != nullptr) + (W8 != nullptr) != 1 || (W8 && !wscale) || (!W8 && wscale)) return fail(c, DTK_ERR_ARG, "%s: exactly one of W | W8 + wscale", who);
  const bool pair = (pro == PRO_RMSNORM && (epi == EPI_QKV || epi == EPI_SWIGLU || epi == EPI_LOGITS || epi == EPI_STORE)) ||
                    (pro == PRO_COPY && (epi == EPI_RESID || epi == EPI_STORE));
  if (!pair) return fail(c, DTK_ERR_ARG, "%s: the step has no launch with prologue %d and epilogue %d", who, pro, epi);
  if (nb != 1 && nb != 2 && nb != 4) return fail(c, DTK_ERR_ARG, "%s: nb %d (1, 2 or 4)", who, nb);
  if (shape < -1 || shape > 3) return fail(c, DTK_ERR_ARG, "%s: shape %d (-1 = the step's choice, 0..3)", who, shape);
  if (N < 1 || K < 8 || (K & 7) || (W8 && (K & 15))) return fail(c, DTK_ERR_ARG, "%s: N >= 1, K a multiple of 8 (16 for fp8 weights)", who);
  if (scratch_fill < 0 || scratch_fill > 255 || d < 0) return fail(c, DTK_ERR_ARG, "%s: scratch_fill is a byte, d >= 0", who);
  if (x_layout != 0 && x_layout != 1) return fail(c, DTK_ERR_ARG, "%s: x_layout %d (0 rows, 1 fragment order)", who, x_layout);
  if (x_layout == 1 && pro == PRO_RMSNORM) return fail(c, DTK_ERR_ARG, "%s: PRO_RMSNORM reads residual streams, which are rows", who);
  if (!X || !pos || !active || (pro == PRO_RMSNORM && !norm_w)) return fail(c, DTK_ERR_ARG, "%s: X, pos, active (and norm_w for PRO_RMSNORM) required", who);
  for (int b = 0; b < nb; ++b)
    if (bs_null && !active[b]) return fail(c, DTK_ERR_ARG, "%s: without a BatchState every slot decodes (slot %d is idle)", who, b);
  if ((size_t)nb * K * 2 + (size_t)nb * 16 * 4 + 64 > (size_t)160 * 1024)
    return fail(c, DTK_ERR_ARG, "%s: %d vectors of K = %d do not fit a CU's 160 KiB of LDS", who, nb, K);
  if (epi == EPI_QKV) {
    if (H < 1 || KVH < 1 || H % KVH) return fail(c, DTK_ERR_ARG, "%s: H %d query heads over KVH %d key / value heads", who, H, KVH);
    if (N != (H + 2 * KVH) * 128 || d != H * 128) return fail(c, DTK_ERR_ARG, "%s: QKV needs N = (H + 2 KVH) * 128 and d = H * 128", who);
    if (T_max < 1) return fail(c, DTK_ERR_ARG, "%s: T_max %d", who, T_max);
    for (int b = 0; b < nb; ++b)
      if (pos[b] < 0 || pos[b] >= T_max) return fail(c, DTK_ERR_ARG, "%s: slot %d: position %d of %d rows", who, b, pos[b], T_max);
    if (!rope_cos || !rope_sin || !q_io || !k_io || !v_io) return fail(c, DTK_ERR_ARG, "%s: QKV needs the rope tables and q / k / v buffers", who);
  } else if (epi == EPI_SWIGLU) {
    if (ff < 8 || (ff & 7) || N != 2 * ff || !y_io) return fail(c, DTK_ERR_ARG, "%s: SWIGLU needs ff a multiple of 8 (as dtk_create), N = 2 ff and y", who);
  } else if (epi == EPI_LOGITS) {
    if (!logits_io) return fail(c, DTK_ERR_ARG, "%s: LOGITS needs the logits buffer", who);
  } else if (!y_io) return fail(c, DTK_ERR_ARG, "%s: RESID / STORE need y", who);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const bool qkv = epi == EPI_QKV;
  const size_t kv_slot = qkv ? (size_t)KVH * T_max * 128 : 0;
  const size_t ny = epi == EPI_SWIGLU ? (size_t)((ff + 31) >> 5) * 512 : ((epi == EPI_STORE || epi == EPI_RESID) ? (size_t)nb * N : 0);
  BatchState hbs; memset(&hbs, 0, sizeof hbs);
  DecState hst[4]; memset(hst, 0, sizeof hst);
  for (int j = 0; j < DTK_MAX_BATCH; ++j) hbs.share_src[j] = -1;
  for (int b = 0; b < nb; ++b) { hbs.active[b] = active[b] ? 1 : 0; hst[b].pos = pos[b]; hst[b].next_pos = pos[b] + 1; }
  OpRun r(c, who, scratch_fill);
  GemvMvArgs g{};
  if (W8) { g.W8 = r.in<uint8_t>(W8, (size_t)N * K); g.wscale = r.in<float>(wscale, N); }
  else g.W = r.in<bf16_t>(W, (size_t)N * K);
  g.X = r.in<bf16_t>(X, x_layout ? (size_t)((K + 31) >> 5) * 512 : (size_t)nb * K);
  g.norm_w = r.in<bf16_t>(pro == PRO_RMSNORM ? norm_w : nullptr, pro == PRO_RMSNORM ? K : 0);
  g.rope_cos = r.in<bf16_t>(qkv ? rope_cos : nullptr, qkv ? (size_t)T_max * 64 : 0);
  g.rope_sin = r.in<bf16_t>(qkv ? rope_sin : nullptr, qkv ? (size_t)T_max * 64 : 0);
  g.st = r.in<DecState>(hst, 4);
  const BatchState* dbs = r.in<BatchState>(&hbs, 1);
  g.bs = bs_null ? nullptr : dbs;
  g.q_out = r.io<bf16_t>(qkv ? q_io : nullptr, qkv ? (size_t)nb * d : 0, "q");
  g.kcache = r.io<bf16_t>(qkv ? k_io : nullptr, (size_t)nb * kv_slot, "k");
  g.vcache = r.io<bf16_t>(qkv ? v_io : nullptr, (size_t)nb * kv_slot, "v");
  g.Y = r.io<bf16_t>(ny ? y_io : nullptr, ny, "y");
  g.logits = r.io<float>(epi == EPI_LOGITS ? logits_io : nullptr, epi == EPI_LOGITS ? (size_t)nb * N : 0, "logits");
  g.N = N; g.K = K; g.ldx = K; g.x_rowmajor = x_layout == 0; g.eps = eps; g.ldy = N; g.kv_slot_stride = kv_slot;
  g.T_max = T_max; g.d = d; g.ff = ff; g.H = H; g.KVH = KVH;
  if (const int rc = r.upload(s)) return rc;      // (hbs and hst live on this frame: upload() waits for the copies)
  {
    MvShapeScope scope(epi, shape);
    launch_gemv_mv(pro, epi, nb, g, s);
  }
  return r.finish(s);
}

// ---- w13.h's host code for the CPU tests: rows [N][K] bf16 <-> planes [N][dtk_w13_row_bytes(K)] + hb[N]; bad[N] = weights below the
// row's window (0 = the row is packed exactly)
int dtk_w13_row_bytes(int K) { return (K < 8 || (K & 7)) ? -1 : (int)w13_row_bytes(K); }
int dtk_w13_pack_host(const uint16_t* W, int N, int K, uint8_t* planes, uint8_t* hb, int32_t* bad) {
  if (!W || !planes || !hb || !bad || N < 1 || K < 8 || (K & 7)) return DTK_ERR_ARG;
  for (int r = 0; r < N; ++r) bad[r] = w13_pack_row(W + (size_t)r * K, K, planes + (size_t)r * w13_row_bytes(K), hb + r);
  return DTK_OK;
}
int dtk_w13_unpack_host(const uint8_t* planes, const uint8_t* hb, int N, int K, uint16_t* W) {
  if (!W || !planes || !hb || N < 1 || K < 8 || (K & 7)) return DTK_ERR_ARG;
  for (int r = 0; r < N; ++r) w13_unpack_row(planes + (size_t)r * w13_row_bytes(K), hb[r], K, W + (size_t)r * K);
  return DTK_OK;
}
int dtk_w13_op_bad_rows(dtk_ctx* c) { return c ? c->w13_op_bad_rows : -1; }
int dtk_w13_flagged_rows(dtk_ctx* c, int role) { return (c && role >= 0 && role < 5 && c->w13_ready) ? (int)c->w13_zrows[role] : -1; }
int dtk_w13_row_bytes_host(const uint16_t* W, int N, int K, uint8_t* bytes) {
  if (!W || !bytes || N < 0 || K < 8 || (K & 7)) return DTK_ERR_ARG;
  for (int r = 0; r < N; ++r) bytes[r] = (uint8_t)w13_row_byte(W + (size_t)r * K, K);
  return DTK_OK;
}

// ---- the batched decode GEMV family alone (dtk_op_gemv_b / dtk_op_gemv_bkp): host operands into the op scratch, the step's own
// launchers (launch_retile / launch_retile_f8, launch_rmsnorm_b, launch_gemv_b, launch_gemv_bkp, launch_resid_norm_b) unchanged
extern "C++" {
namespace {
inline int op_nt_of(int nslots) { const int hi = nslots - 1; return hi < 16 ? 1 : (hi < 32 ? 2 : 4); }   // as dtk_decode_batch_launch: from the highest slot
// the weights as the loader leaves them: the row-major upload (returned) and room for the fragment-major (bf16) or pair-tiled (fp8) copy
// that op_retile makes of it after upload()
const void* op_tiled_weights(OpRun& r, const uint16_t* W, const uint8_t* W8, const float* wscale, int N, int K, GemvBArgs& g) {
  g.N = N; g.K = K;
  if (W8) {
    const uint8_t* dW = r.in<uint8_t>(W8, (size_t)N * K);
    g.W8 = (uint8_t*)r.take(tiled_bytes_f8(N, K)); g.wscale = r.in<float>(wscale, N);
    return dW;
  }
  const bf16_t* dW = r.in<bf16_t>(W, (size_t)N * K);
  g.W = (bf16_t*)r.take(tiled_elems(N, K) * sizeof(bf16_t));
  return dW;
}
void op_retile(const void* rows, const GemvBArgs& g, hipStream_t s) {
  if (g.W8) launch_retile_f8((const uint8_t*)rows, const_cast<uint8_t*>(g.W8), g.N, g.K, s);
  else launch_retile((const bf16_t*)rows, const_cast<bf16_t*>(g.W), g.N, g.K, s);
}
// the 64 slots' flags (slots >= nslots idle) and positions; the host copies live as long as this object, which is beyond upload()
struct OpBatchState {
  BatchState hbs; DecState hst[DTK_MAX_BATCH];
  OpBatchState(OpRun& r, const int32_t* active, const int32_t* pos, int nslots, GemvBArgs& g) {
    memset(&hbs, 0, sizeof hbs); memset(hst, 0, sizeof hst);
    for (int j = 0; j < DTK_MAX_BATCH; ++j) hbs.share_src[j] = -1;
    for (int j = 0; j < nslots; ++j) {
      hbs.active[j] = active[j] ? 1 : 0;
      if (pos) { hst[j].pos = pos[j]; hst[j].next_pos = pos[j] + 1; }
    }
    g.bs = r.in<BatchState>(&hbs, 1); g.st = r.in<DecState>(hst, DTK_MAX_BATCH); g.nt = op_nt_of(nslots);
  }
  OpBatchState(const OpBatchState&) = delete;
};
// X [nslots][K] row-major -> the fragment-major input of 4 column tiles (zero beyond nslots and in the padding of the last k-step)
std::vector<bf16_t> op_x_fragments(const uint16_t* X, int nslots, int K) {
  const int nsteps = (K + 31) >> 5;
  std::vector<bf16_t> h((size_t)4 * nsteps * 512, (bf16_t)0);
  for (int j = 0; j < nslots; ++j)
    for (int k = 0; k < K; ++k) h[host_xtile_off(j, k, nsteps)] = X[(size_t)j * K + k];
  return h;
}
// ... and back: the rows of the first nslots slots
void op_x_rows(const bf16_t* frag, int nslots, int K, uint16_t* X) {
  const int nsteps = (K + 31) >> 5;
  for (int j = 0; j < nslots; ++j)
    for (int k = 0; k < K; ++k) X[(size_t)j * K + k] = frag[host_xtile_off(j, k, nsteps)];
}
}  // namespace
}  // extern "C++"

int dtk_op_gemv_b(dtk_ctx* c, int epi, const uint16_t* W, const uint8_t* W8, const float* wscale, int N, int K,
                  const uint16_t* X, const uint16_t* norm_w, float eps, const int32_t* active, const int32_t* pos, int nslots,
                  int d, int ff, int H, int KVH, int T_max, const uint16_t* rope_cos, const uint16_t* rope_sin,
                  uint16_t* q_io, uint16_t* k_io, uint16_t* v_io, uint16_t* y_io, uint16_t* frag_io, float* logits_io,
                  uint16_t* xn_out, uint32_t* err_out) {
  if (!c || !X || !active || !err_out || (!W == !W8) || (W8 && !wscale)) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_b: null argument, or not exactly one of W / W8 + wscale");
  if (nslots < 1 || nslots > DTK_MAX_BATCH || N < 1 || K < 8 || (K & 7)) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_b: nslots 1..64, N >= 1, K a multiple of 8");
  if (epi != EPI_STORE && epi != EPI_RESID && epi != EPI_QKV && epi != EPI_SWIGLU && epi != EPI_LOGITS) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_b: unknown epilogue %d", epi);
  if (xn_out && !norm_w) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_b: xn_out without norm_w");
  if (epi == EPI_QKV) {
    if (H < 1 || KVH < 1 || H % KVH || N != (H + 2 * KVH) * 128 || d != H * 128 || T_max < 1 || !pos || !rope_cos || !rope_sin || !q_io || !k_io || !v_io)
      return fail(c, DTK_ERR_ARG, "dtk_op_gemv_b: QKV needs N = (H + 2 KVH) * 128, d = H * 128, positions, rope tables and q / k / v buffers");
    for (int j = 0; j < nslots; ++j)
      if (active[j] && (pos[j] < 0 || pos[j] >= T_max)) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_b: slot %d: position %d of %d rows", j, pos[j], T_max);
  } else if (epi == EPI_SWIGLU) {
    if (ff < 8 || (ff & 7) || N != 2 * ff || !y_io || !frag_io) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_b: SWIGLU needs ff a multiple of 8 (as dtk_create), N = 2 ff, y and the fragment buffer");
  } else if (epi == EPI_LOGITS) {
    if (!logits_io) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_b: LOGITS needs the logits buffer");
  } else if (!y_io) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_b: RESID / STORE need y");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, "dtk_op_gemv_b");
  GemvBArgs g{};
  const void* w_rows = op_tiled_weights(r, W, W8, wscale, N, K, g);
  const OpBatchState state(r, active, pos, nslots, g);
  const size_t fe = (size_t)4 * ((K + 31) >> 5) * 512;
  std::vector<bf16_t> hx, hxn(xn_out ? fe : 0);
  const bf16_t *dXr = nullptr, *dn = nullptr;
  bf16_t* dF = nullptr;
  if (norm_w) {      // X = residual streams (zero beyond nslots): k_rmsnorm_b writes the fragments of the active slots
    hx.assign((size_t)DTK_MAX_BATCH * K, (bf16_t)0);
    memcpy(hx.data(), X, (size_t)nslots * K * 2);
    dXr = r.in<bf16_t>(hx.data(), hx.size()); dn = r.in<bf16_t>(norm_w, K);
    g.X = dF = r.out<bf16_t>(xn_out ? hxn.data() : nullptr, fe, "xn");
  } else {
    hx = op_x_fragments(X, nslots, K);
    g.X = r.in<bf16_t>(hx.data(), fe);
  }
  g.ldx = K;
  g.err = r.out<unsigned>(err_out, 1, "err");
  g.d = d; g.ff = ff; g.H = H; g.KVH = KVH; g.T_max = T_max;
  const size_t kv_slot = (size_t)(KVH > 0 ? KVH : 0) * (T_max > 0 ? T_max : 0) * 128, kv = (size_t)DTK_MAX_BATCH * kv_slot;
  const size_t frag_elems = (size_t)4 * ((ff + 31) >> 5) * 512;
  if (epi == EPI_QKV) {
    g.q_out = r.io<bf16_t>(q_io, (size_t)DTK_MAX_BATCH * d, "q"); g.kcache = r.io<bf16_t>(k_io, kv, "k"); g.vcache = r.io<bf16_t>(v_io, kv, "v");
    g.kv_slot_stride = kv_slot; g.rope_cos = r.in<bf16_t>(rope_cos, (size_t)T_max * 64); g.rope_sin = r.in<bf16_t>(rope_sin, (size_t)T_max * 64);
  } else if (epi == EPI_SWIGLU) {
    g.Y = r.io<bf16_t>(frag_io, frag_elems, "frag"); g.ldy = ff;
  } else if (epi == EPI_LOGITS) {
    g.logits = r.io<float>(logits_io, (size_t)DTK_MAX_BATCH * N, "logits");
  } else {
    g.Y = r.io<bf16_t>(y_io, (size_t)DTK_MAX_BATCH * N, "y"); g.ldy = N;
  }
  if (const int rc = r.upload(s)) return rc;
  op_retile(w_rows, g, s);
  if (norm_w) {
    HIPCHK(c, hipMemsetAsync(dF, 0, fe * 2, s));
    launch_rmsnorm_b(dXr, K, dn, dF, K, K, eps, g.bs, 16 * g.nt, s);
  }
  HIPCHK(c, hipMemsetAsync(g.err, 0, 4, s));
  launch_gemv_b(epi, g, s);
  if (const int rc = r.finish(s)) return rc;
  if (epi == EPI_SWIGLU) op_x_rows(frag_io, nslots, ff, y_io);
  if (xn_out) op_x_rows(hxn.data(), nslots, K, xn_out);
  return DTK_OK;
}

int dtk_op_gemv_bkp(dtk_ctx* c, const uint16_t* W, const uint8_t* W8, const float* wscale, int N, int K, const uint16_t* X,
                    const int32_t* active, int nslots, const uint16_t* norm_w, float eps, uint16_t* resid_io, uint16_t* xn_io,
                    float* part_out, uint32_t* err_out) {
  if (!c || !X || !active || !norm_w || !resid_io || !xn_io || !part_out || !err_out || (!W == !W8) || (W8 && !wscale))
    return fail(c, DTK_ERR_ARG, "dtk_op_gemv_bkp: null argument, or not exactly one of W / W8 + wscale");
  if (nslots < 1 || nslots > DTK_MAX_BATCH || N < 1 || K < 8 || (K & 7)) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_bkp: nslots 1..64, N >= 1, K a multiple of 8");
  {   // the step's own question, asked before anything is uploaded or launched (only the shape, the format and the tile count are read)
    GemvBArgs t{};
    float dummy = 0.f;
    t.N = N; t.K = K; t.nt = op_nt_of(nslots); t.kpart = &dummy; t.W8 = W8;
    if (!resid_kparts_covers(t)) return fail(c, DTK_ERR_ARG, "dtk_op_gemv_bkp: N %d, K %d, %d slots, %s weights: not covered by the K-slice kernels", N, K, nslots, W8 ? "fp8" : "bf16");
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, "dtk_op_gemv_bkp");
  GemvBArgs g{};
  const void* w_rows = op_tiled_weights(r, W, W8, wscale, N, K, g);
  const OpBatchState state(r, active, nullptr, nslots, g);
  const std::vector<bf16_t> hx = op_x_fragments(X, nslots, K);
  std::vector<bf16_t> f = op_x_fragments(xn_io, DTK_MAX_BATCH, N);
  const size_t pe = (size_t)8 * DTK_MAX_BATCH * N;
  g.X = r.in<bf16_t>(hx.data(), hx.size()); g.ldx = K;
  float* dP = r.out<float>(part_out, pe, "part");
  bf16_t* dR = r.io<bf16_t>(resid_io, (size_t)DTK_MAX_BATCH * N, "resid");
  const bf16_t* dn = r.in<bf16_t>(norm_w, N);
  bf16_t* dF = r.io<bf16_t>(f.data(), f.size(), "xn");
  g.err = r.out<unsigned>(err_out, 1, "err");
  g.kpart = dP; g.d = N; g.Y = dR; g.ldy = N;
  if (const int rc = r.upload(s)) return rc;
  op_retile(w_rows, g, s);
  HIPCHK(c, hipMemsetAsync(dP, 0xFF, pe * 4, s));
  HIPCHK(c, hipMemsetAsync(g.err, 0, 4, s));
  launch_gemv_bkp(g, s);
  launch_resid_norm_b(dP, dR, N, dn, dF, N, eps, g.bs, 16 * g.nt, s);
  if (const int rc = r.finish(s)) return rc;
  op_x_rows(f.data(), DTK_MAX_BATCH, N, xn_io);
  return DTK_OK;
}

int dtk_op_layernorm(dtk_ctx* c, const uint16_t* X, const uint16_t* w, const uint16_t* b, int M, int D, float eps, uint16_t* Y) {
  if (!c || !X || !w || !b || !Y || D % 8) return fail(c, DTK_ERR_ARG, "dtk_op_layernorm: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, "dtk_op_layernorm");
  const bf16_t* dX = r.in<bf16_t>(X, (size_t)M * D); const bf16_t* dw = r.in<bf16_t>(w, D); const bf16_t* db = r.in<bf16_t>(b, D);
  bf16_t* dY = r.out<bf16_t>(Y, (size_t)M * D, "Y");
  if (const int rc = r.upload(s)) return rc;
  launch_layernorm_rows(dX, D, dw, db, dY, D, M, D, eps, s);
  return r.finish(s);
}

struct OpPen { float pp, fp; const int64_t* ids; int n; };     // dtk_op_sample_pen's own arguments
struct OpDry { const dtk_dry* d; const int64_t* hist; int n; };   // dtk_op_sample_dry's / dtk_op_dry_scan's: the history h[0, n) itself
// a DRY state of the call's own in the op scratch (record, history, empty table and touched list): declared with the op's other buffers,
// ready for launch_dry_scan once upload() and clear() ran.  m_host: where finish() leaves the whole table (or null).  The host copies of
// the record, the length and the history live as long as this object, which is beyond upload()
extern "C++" {
namespace {
struct OpDryState {
  dtk_ctx* c; DryDev rec; DryLen len; std::vector<int32_t> h32; DryScanArgs ds;
  OpDryState(OpRun& r, const OpDry& od, int n_now, int V, uint8_t* m_host) : c(r.c), rec(dry_record(od.d)), len{n_now, 0}, h32(ids32_of(od.hist, od.n)) {
    const int stride = (V + 15) & ~15, cap = od.n > 0 ? od.n : 1;
    ds.dry = r.in<DryDev>(&rec, 1); ds.hist = r.in<int32_t>(od.n > 0 ? h32.data() : nullptr, cap); ds.touched = (int32_t*)r.take(sizeof(int32_t) * cap);
    ds.len = r.in<DryLen>(&len, 1); ds.n_touched = (int32_t*)r.take(sizeof(int32_t)); ds.m = r.out<uint8_t>(m_host, stride, "m");
    ds.hist_stride = cap; ds.m_stride = stride; ds.V = V; ds.bs = nullptr; ds.nslots = 1;
  }
  OpDryState(const OpDryState&) = delete;
  int clear(hipStream_t s) {      // an empty table and touched list (after upload())
    HIPCHK(c, hipMemsetAsync(ds.n_touched, 0, sizeof(int32_t), s));
    HIPCHK(c, hipMemsetAsync(ds.m, 0, (size_t)ds.m_stride, s));
    return DTK_OK;
  }
};
}  // namespace
}  // extern "C++"

// dtk_op_sample_shape's: the sequence's length, its length rules and its bias pairs
struct OpShape { int cur; const dtk_length_ctl* l; const int32_t* ids; const float* val; int n; };
static int op_sample_impl(dtk_ctx* c, const float* logits, int V, int step, int64_t* token_out, float* probs_out, float* lp_out,
                          const dtk_sampling_ext* ext = nullptr, const OpPen* pen = nullptr, const OpDry* dry = nullptr,
                          const OpShape* shp = nullptr) {
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, "dtk_op_sample");
  SampleArgs sa;
  sa.logits = r.in<float>(logits, V); sa.tok_ring = r.out<int64_t>(token_out, 1, "token");
  float2* dlp = r.out<float2>(lp_out, 1, "lp");
  SamplingDev* dsp = (SamplingDev*)r.take(sizeof(SamplingDev));
  // a count table of the call's own, built by the product scatter kernel from the token list
  const int pen_stride = (V + 7) & ~7;
  const PenDev pv{pen ? pen->pp : 0.f, pen ? pen->fp : 0.f};
  const std::vector<int32_t> ids32 = ids32_of(pen ? pen->ids : nullptr, pen ? pen->n : 0);
  int32_t* dids = nullptr; uint16_t* dcnt = nullptr;
  if (pen) {
    sa.pen = r.in<PenDev>(&pv, 1); sa.pen_cnt = dcnt = (uint16_t*)r.take(sizeof(uint16_t) * (size_t)pen_stride); sa.pen_stride = pen_stride;      // advance = 0: nothing is counted
    dids = r.in<int32_t>(pen->n > 0 ? ids32.data() : nullptr, pen->n > 0 ? pen->n : 1);
  }
  std::optional<OpDryState> dst;      // the product scan over the call's own history, then the PN samplers with its table
  if (dry && pen) dst.emplace(r, *dry, dry->n, V, nullptr);
  // a record, a decay table (as far as this length reads it) and a dense bias table of the call's own, filled by the product scatter kernel
  LenDev lrec = len_record(shp ? shp->l : nullptr);
  std::vector<float> mtab(1, 0.f);
  float* dbias = nullptr;
  const int bias_stride = (V + 7) & ~7;
  if (shp && pen) {
    for (int i = 0; i < shp->n; ++i) lrec.n_bias += shp->val[i] != 0.f;
    if (lrec.decay_begin != DTK_LEN_NO_DECAY) {
      const long k = (long)shp->cur - lrec.start - lrec.decay_begin;
      mtab.resize((size_t)(k > 0 ? k + 1 : 1));
      len_table(shp->l->decay_factor, mtab.data(), (int)mtab.size());
    }
    sa.len = r.in<LenDev>(&lrec, 1); sa.len_m = r.in<float>(mtab.data(), mtab.size()); sa.len_m_stride = (int)mtab.size();
    sa.bias = dbias = (float*)r.take(sizeof(float) * (size_t)bias_stride); sa.bias_stride = bias_stride; sa.len_cur = shp->cur;
  }
  if (probs_out) r.res.push_back({c->probs_dev, probs_out, (size_t)V * 4, "probs", false});      // (the context's own buffer, not in the scratch)
  if (const int rc = r.upload(s)) return rc;
  if (pen) {
    HIPCHK(c, hipMemsetAsync(dcnt, 0, sizeof(uint16_t) * (size_t)pen_stride, s));
    launch_count_scatter(dids, pen->n, dcnt, V, s);
  }
  if (dbias) {
    HIPCHK(c, hipMemsetAsync(dbias, 0, sizeof(float) * (size_t)bias_stride, s));
    launch_bias_scatter(shp->ids, shp->val, shp->n, dbias, V, s);
  }
  ExtDev xd{};
  if (ext) {      // the context's configuration with the call's own (min_p, epsilon_cutoff)
    xd = ext_dev(ext);
    HIPCHK(c, hipMemcpyAsync(dsp, c->sp, sizeof(SamplingDev), hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(reinterpret_cast<char*>(dsp) + offsetof(SamplingDev, qmin), &xd, sizeof xd, hipMemcpyHostToDevice, s));
  }
  sa.V = V; sa.sp = c->sp; sa.st = c->st; sa.embed = c->embed; sa.x = c->x; sa.d = c->d;
  sa.ring = 1; sa.probs_out = probs_out ? c->probs_dev : nullptr; sa.advance = 0;
  sa.step_override = step; sa.bs = nullptr; sa.logits_stride = 0; sa.nslots = 1; sa.mb = c->smb;
  sa.lp_ring = lp_out ? dlp : nullptr;
  if (ext) { sa.sp = dsp; sa.trunc = (xd.qmin != 0 || xd.eps != 0.f) ? 1 : 0; }
  else sa.trunc = c->trunc_single ? 1 : 0;
  if (dst) {
    if (const int rc = dst->clear(s)) return rc;
    launch_dry_scan(dst->ds, s);
    sa.dry = dst->ds.dry; sa.dry_m = dst->ds.m; sa.dry_stride = dst->ds.m_stride;
  }
  const bool needs_topk = c->sampling.do_sample && c->sampling.top_k > 0 && c->sampling.top_k < V;
  if (sample_mb_preferred(V, c->sampling.do_sample != 0) && !needs_topk && !getenv("DTK_SAMPLER")) launch_sample_mb(sa, s); else launch_sample(sa, s);
  return r.finish(s);
}

int dtk_op_sample(dtk_ctx* c, const float* logits, int V, int step, int64_t* token_out, float* probs_out) {
  if (!c || !logits || !token_out || V < 1 || V > c->V) return fail(c, DTK_ERR_ARG, "dtk_op_sample: bad argument");
  return op_sample_impl(c, logits, V, step, token_out, probs_out, nullptr);
}

// dtk_op_sample + lp_out[2] = (logprob, sample_logprob) of the token: the LP sampler instantiations over given logits.  The row may
// be longer than the context's own vocabulary (any V the samplers take: <= 262 144) as long as probs_out is null
int dtk_op_sample_lp(dtk_ctx* c, const float* logits, int V, int step, int64_t* token_out, float* probs_out, float* lp_out) {
  if (!c || !logits || !token_out || !lp_out || V < 1 || V > DTK_SAMPLE_MB_MAX_SLICES * 8192 || (probs_out && V > c->V))
    return fail(c, DTK_ERR_ARG, "dtk_op_sample_lp: bad argument");
  if (!c->logprobs) return fail(c, DTK_ERR_ARG, "dtk_op_sample_lp: the context does not compute log-probabilities (dtk_set_option \"logprobs\", 1)");
  return op_sample_impl(c, logits, V, step, token_out, probs_out, lp_out);
}

// dtk_op_sample_lp under the context's configuration with the call's own (min_p, epsilon_cutoff): the TR sampler instantiations (both 0:
// the kernels dtk_op_sample_lp runs).  lp_out may be null (the LP = false kernels; no "logprobs" option needed then)
int dtk_op_sample_ext(dtk_ctx* c, const float* logits, int V, int step, int64_t* token_out, float* probs_out, float* lp_out,
                      const dtk_sampling_ext* ext) {
  if (!c || !logits || !token_out || V < 1 || V > DTK_SAMPLE_MB_MAX_SLICES * 8192 || (probs_out && V > c->V))
    return fail(c, DTK_ERR_ARG, "dtk_op_sample_ext: bad argument");
  if (const int rc = ext_check(c, ext, "dtk_op_sample_ext")) return rc;
  if (lp_out && !c->logprobs) return fail(c, DTK_ERR_ARG, "dtk_op_sample_ext: the context does not compute log-probabilities (dtk_set_option \"logprobs\", 1)");
  return op_sample_impl(c, logits, V, step, token_out, probs_out, lp_out, ext);
}

// dtk_op_sample_ext (ext may be null: the context's own min_p / epsilon_cutoff) with a presence / frequency penalty over the counts of a
// given token list: the PN sampler instantiations and k_count_scatter, whatever the two values are
int dtk_op_sample_pen(dtk_ctx* c, const float* logits, int V, int step, int64_t* token_out, float* probs_out, float* lp_out,
                      const dtk_sampling_ext* ext, float presence, float frequency, const int64_t* counted_ids, int n_counted) {
  if (!c || !logits || !token_out || V < 1 || V > DTK_SAMPLE_MB_MAX_SLICES * 8192 || (probs_out && V > c->V) || n_counted < 0 ||
      n_counted > 65535 || (n_counted > 0 && !counted_ids))
    return fail(c, DTK_ERR_ARG, "dtk_op_sample_pen: bad argument");
  if (ext) if (const int rc = ext_check(c, ext, "dtk_op_sample_pen")) return rc;
  if (const int rc = pen_check(c, presence, frequency, 0, "dtk_op_sample_pen")) return rc;
  for (int i = 0; i < n_counted; ++i)
    if (counted_ids[i] < 0 || counted_ids[i] >= V) return fail(c, DTK_ERR_ARG, "dtk_op_sample_pen: counted id %lld outside [0, %d)", (long long)counted_ids[i], V);
  if (lp_out && !c->logprobs) return fail(c, DTK_ERR_ARG, "dtk_op_sample_pen: the context does not compute log-probabilities (dtk_set_option \"logprobs\", 1)");
  const OpPen pn{presence, frequency, counted_ids, n_counted};
  return op_sample_impl(c, logits, V, step, token_out, probs_out, lp_out, ext, &pn);
}

static int op_dry_check(dtk_ctx* c, const dtk_dry* d, int V, const int64_t* hist, int n, const char* who) {
  if (const int rc = dry_check(c, d, V, who)) return rc;
  if (n < 0 || n > 65535 || (n > 0 && !hist)) return fail(c, DTK_ERR_ARG, "%s: a history of 0 .. 65535 ids", who);
  for (int i = 0; i < n; ++i)
    if (hist[i] < 0 || hist[i] >= V) return fail(c, DTK_ERR_ARG, "%s: history id %lld outside [0, %d)", who, (long long)hist[i], V);
  return DTK_OK;
}

// dtk_op_sample_pen with DRY over a given history h[0, n) (dry->start is not used: the history is given as it stands): k_dry_scan, then
// the PN sampler instantiations with both the count table and the match table, whatever the values are
int dtk_op_sample_dry(dtk_ctx* c, const float* logits, int V, int step, int64_t* token_out, float* probs_out, float* lp_out,
                      const dtk_sampling_ext* ext, float presence, float frequency, const int64_t* counted_ids, int n_counted,
                      const int64_t* history, int n_history, const dtk_dry* dry) {
  if (!c || !logits || !token_out || V < 1 || V > DTK_SAMPLE_MB_MAX_SLICES * 8192 || (probs_out && V > c->V) || n_counted < 0 ||
      n_counted > 65535 || (n_counted > 0 && !counted_ids))
    return fail(c, DTK_ERR_ARG, "dtk_op_sample_dry: bad argument");
  if (ext) if (const int rc = ext_check(c, ext, "dtk_op_sample_dry")) return rc;
  if (const int rc = pen_check(c, presence, frequency, 0, "dtk_op_sample_dry")) return rc;
  if (const int rc = op_dry_check(c, dry, V, history, n_history, "dtk_op_sample_dry")) return rc;
  for (int i = 0; i < n_counted; ++i)
    if (counted_ids[i] < 0 || counted_ids[i] >= V) return fail(c, DTK_ERR_ARG, "dtk_op_sample_dry: counted id %lld outside [0, %d)", (long long)counted_ids[i], V);
  if (lp_out && !c->logprobs) return fail(c, DTK_ERR_ARG, "dtk_op_sample_dry: the context does not compute log-probabilities (dtk_set_option \"logprobs\", 1)");
  const OpPen pn{presence, frequency, counted_ids, n_counted};
  const OpDry od{dry, history, n_history};
  return op_sample_impl(c, logits, V, step, token_out, probs_out, lp_out, ext, &pn, &od);
}

// dtk_op_sample_dry at sequence length cur with a dtk_length_ctl and bias pairs: k_bias_scatter, k_dry_scan, then the PN sampler
// instantiations with the count table, the match table, the decay table and the bias table, whatever the values are
int dtk_op_sample_shape(dtk_ctx* c, const float* logits, int V, int step, int64_t* token_out, float* probs_out, float* lp_out,
                        const dtk_sampling_ext* ext, float presence, float frequency, const int64_t* counted_ids, int n_counted,
                        const int64_t* history, int n_history, const dtk_dry* dry, int cur, const dtk_length_ctl* l,
                        const int32_t* bias_ids, const float* bias_values, int n_bias) {
  if (!c || !logits || !token_out || V < 1 || V > DTK_SAMPLE_MB_MAX_SLICES * 8192 || (probs_out && V > c->V) || n_counted < 0 ||
      n_counted > 65535 || (n_counted > 0 && !counted_ids) || cur < 0 || cur > (1 << 20))
    return fail(c, DTK_ERR_ARG, "dtk_op_sample_shape: bad argument");
  if (ext) if (const int rc = ext_check(c, ext, "dtk_op_sample_shape")) return rc;
  if (const int rc = pen_check(c, presence, frequency, 0, "dtk_op_sample_shape")) return rc;
  if (const int rc = op_dry_check(c, dry, V, history, n_history, "dtk_op_sample_shape")) return rc;
  if (const int rc = len_check(c, l, V, "dtk_op_sample_shape")) return rc;
  if (const int rc = bias_check(c, bias_ids, bias_values, n_bias, V, "dtk_op_sample_shape")) return rc;
  for (int i = 0; i < n_counted; ++i)
    if (counted_ids[i] < 0 || counted_ids[i] >= V) return fail(c, DTK_ERR_ARG, "dtk_op_sample_shape: counted id %lld outside [0, %d)", (long long)counted_ids[i], V);
  if (lp_out && !c->logprobs) return fail(c, DTK_ERR_ARG, "dtk_op_sample_shape: the context does not compute log-probabilities (dtk_set_option \"logprobs\", 1)");
  const OpPen pn{presence, frequency, counted_ids, n_counted};
  const OpDry od{dry, history, n_history};
  const OpShape sh{cur, l, bias_ids, bias_values, n_bias};
  return op_sample_impl(c, logits, V, step, token_out, probs_out, lp_out, ext, &pn, &od, &sh);
}

// k_dry_scan alone over a given history; with history2, a second scan of that history on the state the first one left (table and
// touched list), as two consecutive steps of a sequence do.  The result is read from the WHOLE table behind the last scan: every id
// with M != 0 in ascending order, so an entry a scan failed to clear shows.  Returns their number (the first n_max go out) or an error
int dtk_op_dry_scan(dtk_ctx* c, int V, const int64_t* history, int n_history, const int64_t* history2, int n_history2, const dtk_dry* dry,
                    int32_t* ids_out, uint8_t* m_out, int n_max) {
  if (!c || V < 1 || V > DTK_SAMPLE_MB_MAX_SLICES * 8192 || n_max < 0 || (n_max > 0 && (!ids_out || !m_out)))
    return fail(c, DTK_ERR_ARG, "dtk_op_dry_scan: bad argument");
  if (const int rc = op_dry_check(c, dry, V, history, n_history, "dtk_op_dry_scan")) return rc;
  if (history2) if (const int rc = op_dry_check(c, dry, V, history2, n_history2, "dtk_op_dry_scan")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int cap = history2 && n_history2 > n_history ? n_history2 : n_history;
  std::vector<int64_t> first(history, history + n_history);
  first.resize((size_t)cap, 0);      // (room for the longer of the two; the length says what counts)
  std::vector<uint8_t> tab((size_t)((V + 15) & ~15));
  OpRun r(c, "dtk_op_dry_scan");
  OpDryState st(r, OpDry{dry, first.data(), cap}, n_history, V, tab.data());
  if (const int rc = r.upload(s)) return rc;
  if (const int rc = st.clear(s)) return rc;
  launch_dry_scan(st.ds, s);
  if (history2) {      // the second step's history and length over the state the first scan left
    HIPCHK(c, hipStreamSynchronize(s));
    const std::vector<int32_t> h32 = ids32_of(history2, n_history2);
    const DryLen l2{n_history2, 0};
    if (n_history2 > 0) HIPCHK(c, hipMemcpy(st.ds.hist, h32.data(), sizeof(int32_t) * h32.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(st.ds.len, &l2, sizeof l2, hipMemcpyHostToDevice));
    launch_dry_scan(st.ds, s);
  }
  if (const int rc = r.finish(s)) return rc;
  int k = 0;
  for (int t = 0; t < V; ++t)
    if (tab[(size_t)t]) { if (k < n_max) { ids_out[k] = t; m_out[k] = tab[(size_t)t]; } ++k; }
  return k;
}

// dtk_set_guidance's two mixing kernels on a pair of the call's own: the rows lie at stride V as two slots' rows do (row 0 = zu, row 1 =
// zc, which becomes out: the guard bytes lie behind it), the pair is (1, 0), the launch shape is launch_cfg_mix's for that V
int dtk_op_cfg_mix(dtk_ctx* c, const float* zc, const float* zu, int V, float scale, float* out, float* lse_out) {
  if (!c || !zc || !zu || !out || !lse_out || V < 2 || V > DTK_SAMPLE_MB_MAX_SLICES * 8192 || !std::isfinite(scale) || scale < 0.f || scale > 100.f)
    return fail(c, DTK_ERR_ARG, "dtk_op_cfg_mix: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, "dtk_op_cfg_mix", 0x5a);
  std::vector<float> rows((size_t)2 * V);
  memcpy(rows.data(), zu, sizeof(float) * (size_t)V);
  memcpy(rows.data() + V, zc, sizeof(float) * (size_t)V);
  const CfgPair pair{1, 0, scale, 0};
  CfgArgs g;
  g.logits = (float*)r.take(sizeof(float) * 2 * (size_t)V + OpRun::GUARD);
  r.ins.push_back({g.logits, rows.data(), sizeof(float) * 2 * (size_t)V});
  r.res.push_back({g.logits + V, out, sizeof(float) * (size_t)V, "out", false});
  g.V = V; g.stride = V; g.pairs = r.in<CfgPair>(&pair, 1); g.n_pairs = 1; g.bs = nullptr;
  g.part = (float2*)r.take(sizeof(float2) * 2 * DTK_CFG_MAX_SLICES);
  g.lse = reinterpret_cast<float2*>(r.out<float>(lse_out, 2, "lse"));
  if (const int rc = r.upload(s)) return rc;
  launch_cfg_mix(g, s);
  return r.finish(s);
}

// dtk_spec_begin(.., DTK_SPEC_LOOKUP)'s lookup alone: k_spec_draft over a history of the call's own, nothing but the drafts written
int dtk_op_spec_lookup(dtk_ctx* c, const int32_t* ids, int len, int K, int max_ngram, int T_max, int32_t* drafts_out, int* n_out) {
  if (!c || (!ids && len > 0) || len < 0 || K < 1 || K > 3 || max_ngram < 1 || max_ngram > DTK_SPEC_MAX_NGRAM || T_max < len || T_max < 1 || !drafts_out || !n_out)
    return fail(c, DTK_ERR_ARG, "dtk_op_spec_lookup: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, "dtk_op_spec_lookup", 0x5a);
  int32_t res[7] = {-1, -1, -1, -1, 0, 0, 0};
  SpecArgs a{};
  a.hist = r.in<int32_t>(len > 0 ? ids : nullptr, (size_t)(len > 0 ? len : 1));
  a.table = nullptr; a.K = K; a.max_ngram = max_ngram; a.NV = K + 1; a.T_max = T_max; a.V = c->V;
  a.len_override = len;
  a.drafts_out = r.out<int32_t>(res, 7, "drafts");
  if (const int rc = r.upload(s)) return rc;
  launch_spec_draft(a, s);
  if (const int rc = r.finish(s)) return rc;
  for (int i = 0; i < 4; ++i) drafts_out[i] = res[i];
  *n_out = res[4];
  return DTK_OK;
}

// the lookup with a corpus: k_spec_corpus + k_spec_draft as a step launches them, on a history, a corpus, block results and a SpecDev of
// the call's own (the kernels read the corpus through the record, as in a step)
int dtk_op_spec_lookup_corpus(dtk_ctx* c, const int32_t* ids, int len, const int32_t* corpus, int n_corpus, int K, int max_ngram, int T_max,
                              int32_t* drafts_out, int* n_out, int* source_out, int* ngram_out) {
  if (!c || (!ids && len > 0) || len < 0 || (!corpus && n_corpus > 0) || n_corpus < 0 || K < 1 || K > 3 || max_ngram < 1 ||
      max_ngram > DTK_SPEC_MAX_NGRAM || T_max < len || T_max < 1 || !drafts_out || !n_out || !source_out || !ngram_out)
    return fail(c, DTK_ERR_ARG, "dtk_op_spec_lookup_corpus: bad argument");
  if (n_corpus > DTK_SPEC_CORPUS_MAX) return fail(c, DTK_ERR_RANGE, "dtk_op_spec_lookup_corpus: a corpus of %d entries exceeds DTK_SPEC_CORPUS_MAX = %d", n_corpus, DTK_SPEC_CORPUS_MAX);
  for (int i = 0; i < n_corpus; ++i)
    if (corpus[i] >= c->V) return fail(c, DTK_ERR_ARG, "dtk_op_spec_lookup_corpus: corpus id %d at entry %d", corpus[i], i);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, "dtk_op_spec_lookup_corpus", 0x5a);
  int32_t res[7] = {-1, -1, -1, -1, 0, 0, 0};
  SpecDev sd{};
  sd.K = K; sd.NV = K + 1; sd.max_ngram = max_ngram; sd.use_table = 0; sd.corpus_len = n_corpus;
  SpecArgs a{};
  a.hist = r.in<int32_t>(len > 0 ? ids : nullptr, (size_t)(len > 0 ? len : 1));
  sd.corpus = r.in<int32_t>(n_corpus > 0 ? corpus : nullptr, (size_t)(n_corpus > 0 ? n_corpus : 1));
  sd.corpus_best = r.out<unsigned long long>(nullptr, DTK_SPEC_CORPUS_BLOCKS, "block results");
  a.sd = r.in<SpecDev>(&sd, 1);
  a.table = nullptr; a.T_max = T_max; a.V = c->V;
  a.len_override = len;
  a.drafts_out = r.out<int32_t>(res, 7, "drafts");
  if (const int rc = r.upload(s)) return rc;
  if (n_corpus > 0) launch_spec_corpus(a, s);
  launch_spec_draft(a, s);
  if (const int rc = r.finish(s)) return rc;
  for (int i = 0; i < 4; ++i) drafts_out[i] = res[i];
  *n_out = res[4]; *source_out = res[5]; *ngram_out = res[6];
  return DTK_OK;
}

// dtk_set_option "top_logprobs"'s selection alone, on rows of the call's own: kernel 1 = k_top_logits, 2 = k_top_slice + k_top_merge
// with slices of L, through the shipped launchers.  The rows are the slots of a batched step (record index 0 of a ring of one);
// active / forced (NULL: every row active / none forced) are the BatchState flags and DecState::force_plus1 the kernels read.
// ids_out / z_out [rows][DTK_MAX_TOP] are uploaded first: what a kernel does not write (an inactive row, entries >= k) comes back as
// the caller left it
int dtk_op_top_logits(dtk_ctx* c, const float* logits, int rows, int V, int k, int kernel, int L, const int32_t* active, const int32_t* forced,
                      int32_t* ids_out, float* z_out) {
  if (!c || !logits || !ids_out || !z_out || rows < 1 || rows > DTK_MAX_BATCH || V < 1 || V > DTK_TOP_MAX_SLICES * DTK_TOP_MAX_L || k < 1 ||
      k > DTK_MAX_TOP || k > V || (kernel != 1 && kernel != 2))
    return fail(c, DTK_ERR_ARG, "dtk_op_top_logits: bad argument (rows 1..%d, V 1..%d, k 1..%d and <= V, kernel 1 or 2)", DTK_MAX_BATCH,
                DTK_TOP_MAX_SLICES * DTK_TOP_MAX_L, DTK_MAX_TOP);
  if (kernel == 2 && !top_sliced_ok(V, L))
    return fail(c, DTK_ERR_ARG, "dtk_op_top_logits: L must be 1..%d with at most %d slices of V = %d", DTK_TOP_MAX_L, DTK_TOP_MAX_SLICES, V);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  OpRun r(c, "dtk_op_top_logits", 0x5a);
  BatchState hbs; DecState hst[DTK_MAX_BATCH];
  memset(&hbs, 0, sizeof hbs); memset(hst, 0, sizeof hst);
  for (int j = 0; j < DTK_MAX_BATCH; ++j) hbs.share_src[j] = -1;
  for (int j = 0; j < rows; ++j) { hbs.active[j] = (!active || active[j]) ? 1 : 0; hst[j].force_plus1 = (forced && forced[j]) ? 1 : 0; }
  std::vector<TopRec> recs((size_t)rows);
  for (int j = 0; j < rows; ++j)
    for (int i = 0; i < DTK_MAX_TOP; ++i) { recs[(size_t)j].id[i] = ids_out[(size_t)j * DTK_MAX_TOP + i]; recs[(size_t)j].z[i] = z_out[(size_t)j * DTK_MAX_TOP + i]; }
  TopArgs t;
  t.logits = r.in<float>(logits, (size_t)rows * V); t.V = V; t.logits_stride = V;
  t.bs = r.in<BatchState>(&hbs, 1); t.st = r.in<DecState>(hst, DTK_MAX_BATCH); t.nslots = rows; t.ring = 1; t.k = k;
  t.top_ring = r.io<TopRec>(recs.data(), (size_t)rows, "records");
  if (kernel == 2) { t.L = L; t.scratch = (TopRec*)r.take(sizeof(TopRec) * (size_t)rows * DTK_TOP_MAX_SLICES); }
  if (const int rc = r.upload(s)) return rc;
  if (kernel == 2) launch_top_sliced(t, s); else launch_top_logits(t, s);
  if (const int rc = r.finish(s)) return rc;
  for (int j = 0; j < rows; ++j)
    for (int i = 0; i < DTK_MAX_TOP; ++i) { ids_out[(size_t)j * DTK_MAX_TOP + i] = recs[(size_t)j].id[i]; z_out[(size_t)j * DTK_MAX_TOP + i] = recs[(size_t)j].z[i]; }
  return DTK_OK;
}

}  // extern "C"
#pragma GCC visibility pop
