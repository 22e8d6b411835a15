// dtk_api.hip — the C ABI (include/dtk.h): context, weight registry, ViT / prefill /
// decode orchestration, hipGraph capture of the per-token decode step.
//
// Reference call sites this replaces (all Python in potamides/DeTikZify):
//   DetikzifyVisionModel.forward / get_intermediate_layers  v1/modeling_detikzify.py:63-72
//   DetikzifyModel.get_vision_features + mm_projector        v1/modeling_detikzify.py:132-137,163
//   embedding splice                                          v1/modeling_detikzify.py:158-189
//   LlamaModel.forward / lm_head                              v1/modeling_detikzify.py:191-200,250-257
//   HF GenerationMixin._sample loop body                      via infer/generate.py:218-227
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "dtk_ctx.h"
#include "w13.h"
#include "mx_quant.h"

int& dtk_lds_attr_error(int device) {     // common.h: set by a launcher whose hipFuncSetAttribute was refused, per device
  static int e[65] = {};
  return e[(device >= 0 && device < 64) ? device : 64];
}

namespace {

thread_local std::string g_create_error;
// dtk_last_error is per calling thread (ABI 6): the engine's loop thread, reward threads inside dtk_vit_encode and a caller's own
// thread may all fail on one context; each reads the text of ITS failed call
thread_local std::string g_thread_error;
thread_local const void* g_thread_error_ctx = nullptr;

}  // namespace

// ---- dtk_ctx.h's helpers (shared with dtk_ops.hip)
int fail(dtk_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) {
    { std::lock_guard<std::mutex> g(c->err_mu); c->err = buf; }
    g_thread_error = buf;
    g_thread_error_ctx = c;
  } else {
    g_create_error = buf;
  }
  return code;
}

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

uint16_t host_f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
float host_bf2f(uint16_t h) {
  uint32_t u = ((uint32_t)h) << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
float host_h2f(uint16_t h) {
  const uint32_t sign = (h >> 15) & 1u, exp = (h >> 10) & 0x1fu, man = h & 0x3ffu;
  float v;
  if (exp == 0) v = ldexpf((float)man, -24);
  else if (exp == 31) v = man ? NAN : INFINITY;
  else v = ldexpf((float)(man | 0x400u), (int)exp - 25);
  return sign ? -v : v;
}

namespace {

// ---- arena planning: first pass sums sizes, second pass hands out pointers
struct Planner {
  size_t off = 0;
  unsigned char* base = nullptr;
  template <typename T>
  T* take(size_t n_elems) {
    off = align_up(off, 256);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n_elems * sizeof(T);
    return p;
  }
};

void add_tensor(dtk_ctx* c, const std::string& name, bf16_t* ptr, int64_t rows, int64_t cols,
                int64_t stride, float scale, float offset) {
  TensorEntry t;
  t.name = name; t.ptr = ptr; t.rows = rows; t.cols = cols; t.stride = stride;
  t.synth_scale = scale; t.synth_offset = offset;
  c->tindex[name] = (int)c->tensors.size();
  c->tensors.push_back(t);
}

// Lays out every device buffer.  Called twice (size pass with base == nullptr, then for real).
void plan(dtk_ctx* c, Planner& P, bool reg) {
  const int d = c->d, L = c->L, ff = c->ff, V = c->V, T = c->Tmax;
  const int kvd = c->KVH * c->hd, qkvn = d + 2 * kvd;   // fused QKV rows: [H q heads | KVH k heads | KVH v heads] x hd
  const int D = c->vD, N = c->vN, mlp = c->vMlp;
  const float ws = 0.02f;
  auto R = [&](const std::string& n, bf16_t* p, int64_t r, int64_t cl, int64_t st, float sc,
               float of) { if (reg) add_tensor(c, n, p, r, cl, st, sc, of); };
  // ---- decoder weights
  c->embed = P.take<bf16_t>((size_t)V * d);
  R("model.embed_tokens.weight", c->embed, V, d, d, ws, 0.f);
  if (reg) c->layers.resize(L);
  for (int i = 0; i < L; ++i) {
    LayerW w;
    w.ln1 = P.take<bf16_t>(d);
    w.wqkv = P.take<bf16_t>((size_t)qkvn * d);
    w.wo = P.take<bf16_t>((size_t)d * d);
    w.ln2 = P.take<bf16_t>(d);
    w.wgu = P.take<bf16_t>((size_t)2 * ff * d);
    w.wdown = P.take<bf16_t>((size_t)d * ff);
    if (reg) {
      c->layers[i] = w;
      const std::string p = "model.layers." + std::to_string(i) + ".";
      R(p + "input_layernorm.weight", w.ln1, 1, d, d, 0.1f, 1.f);
      R(p + "self_attn.q_proj.weight", w.wqkv, d, d, d, ws, 0.f);
      R(p + "self_attn.k_proj.weight", w.wqkv + (size_t)d * d, kvd, d, d, ws, 0.f);
      R(p + "self_attn.v_proj.weight", w.wqkv + (size_t)(d + kvd) * d, kvd, d, d, ws, 0.f);
      R(p + "self_attn.o_proj.weight", w.wo, d, d, d, ws, 0.f);
      R(p + "post_attention_layernorm.weight", w.ln2, 1, d, d, 0.1f, 1.f);
      R(p + "mlp.gate_proj.weight", w.wgu, ff, d, d, ws, 0.f);
      R(p + "mlp.up_proj.weight", w.wgu + (size_t)ff * d, ff, d, d, ws, 0.f);
      R(p + "mlp.down_proj.weight", w.wdown, d, ff, ff, ws, 0.f);
    }
  }
  c->final_norm = P.take<bf16_t>(d);
  R("model.norm.weight", c->final_norm, 1, d, d, 0.1f, 1.f);
  c->lm_head = P.take<bf16_t>((size_t)V * d);
  R("lm_head.weight", c->lm_head, V, d, d, ws, 0.f);
  c->mm_w = P.take<bf16_t>((size_t)d * c->cfg.concat_patches * D);
  c->mm_b = P.take<bf16_t>(d);
  R("model.mm_projector.weight", c->mm_w, d, (int64_t)c->cfg.concat_patches * D,
    (int64_t)c->cfg.concat_patches * D, ws, 0.f);
  if (c->proj_bias) R("model.mm_projector.bias", c->mm_b, 1, d, d, 0.01f, 0.f);   // v2 connector is bias-free
  const int hd2 = c->hd / 2;
  c->rope_cos = P.take<bf16_t>((size_t)T * hd2);
  c->rope_sin = P.take<bf16_t>((size_t)T * hd2);
  R("rope.cos", c->rope_cos, T, hd2, hd2, 0.f, 0.f);
  R("rope.sin", c->rope_sin, T, hd2, hd2, 0.f, 0.f);
  // ---- vision tower (timm VisionTransformer state-dict names)
  const std::string vp = "vision_model.";
  c->pe_w = P.take<bf16_t>((size_t)D * c->vPatchLd);
  c->pe_b = P.take<bf16_t>(D);
  c->pos_embed = P.take<bf16_t>((size_t)N * D);
  R(vp + "patch_embed.proj.weight", c->pe_w, D, c->vPatchK, c->vPatchLd, ws, 0.f);
  R(vp + "patch_embed.proj.bias", c->pe_b, 1, D, D, 0.01f, 0.f);
  R(vp + "pos_embed", c->pos_embed, N, D, D, ws, 0.f);
  if (reg) c->vblocks.resize(c->vDepth);
  for (int i = 0; i < c->vDepth; ++i) {
    VitBlockW w;
    w.n1w = P.take<bf16_t>(D); w.n1b = P.take<bf16_t>(D);
    w.qkvw = P.take<bf16_t>((size_t)3 * D * D); w.qkvb = P.take<bf16_t>(3 * D);
    w.projw = P.take<bf16_t>((size_t)D * D); w.projb = P.take<bf16_t>(D);
    w.n2w = P.take<bf16_t>(D); w.n2b = P.take<bf16_t>(D);
    w.fc1w = P.take<bf16_t>((size_t)mlp * D); w.fc1b = P.take<bf16_t>(mlp);
    w.fc2w = P.take<bf16_t>((size_t)D * mlp); w.fc2b = P.take<bf16_t>(D);
    if (reg) {
      c->vblocks[i] = w;
      const std::string p = vp + "blocks." + std::to_string(i) + ".";
      R(p + "norm1.weight", w.n1w, 1, D, D, 0.1f, 1.f);
      R(p + "norm1.bias", w.n1b, 1, D, D, 0.01f, 0.f);
      R(p + "attn.qkv.weight", w.qkvw, 3 * D, D, D, ws, 0.f);
      R(p + "attn.qkv.bias", w.qkvb, 1, 3 * D, 3 * D, 0.01f, 0.f);
      R(p + "attn.proj.weight", w.projw, D, D, D, ws, 0.f);
      R(p + "attn.proj.bias", w.projb, 1, D, D, 0.01f, 0.f);
      R(p + "norm2.weight", w.n2w, 1, D, D, 0.1f, 1.f);
      R(p + "norm2.bias", w.n2b, 1, D, D, 0.01f, 0.f);
      R(p + "mlp.fc1.weight", w.fc1w, mlp, D, D, ws, 0.f);
      R(p + "mlp.fc1.bias", w.fc1b, 1, mlp, mlp, 0.01f, 0.f);
      R(p + "mlp.fc2.weight", w.fc2w, D, mlp, mlp, ws, 0.f);
      R(p + "mlp.fc2.bias", w.fc2b, 1, D, D, 0.01f, 0.f);
    }
  }
  c->vnorm_w = P.take<bf16_t>(D); c->vnorm_b = P.take<bf16_t>(D);
  R(vp + "norm.weight", c->vnorm_w, 1, D, D, 0.1f, 1.f);
  R(vp + "norm.bias", c->vnorm_b, 1, D, D, 0.01f, 0.f);
  c->ap_latent = P.take<bf16_t>(D);
  c->ap_qw = P.take<bf16_t>((size_t)D * D); c->ap_qb = P.take<bf16_t>(D);
  c->ap_kvw = P.take<bf16_t>((size_t)2 * D * D); c->ap_kvb = P.take<bf16_t>(2 * D);
  c->ap_pw = P.take<bf16_t>((size_t)D * D); c->ap_pb = P.take<bf16_t>(D);
  c->ap_nw = P.take<bf16_t>(D); c->ap_nb = P.take<bf16_t>(D);
  c->ap_f1w = P.take<bf16_t>((size_t)mlp * D); c->ap_f1b = P.take<bf16_t>(mlp);
  c->ap_f2w = P.take<bf16_t>((size_t)D * mlp); c->ap_f2b = P.take<bf16_t>(D);
  R(vp + "attn_pool.latent", c->ap_latent, 1, D, D, ws, 0.f);
  R(vp + "attn_pool.q.weight", c->ap_qw, D, D, D, ws, 0.f);
  R(vp + "attn_pool.q.bias", c->ap_qb, 1, D, D, 0.01f, 0.f);
  R(vp + "attn_pool.kv.weight", c->ap_kvw, 2 * D, D, D, ws, 0.f);
  R(vp + "attn_pool.kv.bias", c->ap_kvb, 1, 2 * D, 2 * D, 0.01f, 0.f);
  R(vp + "attn_pool.proj.weight", c->ap_pw, D, D, D, ws, 0.f);
  R(vp + "attn_pool.proj.bias", c->ap_pb, 1, D, D, 0.01f, 0.f);
  R(vp + "attn_pool.norm.weight", c->ap_nw, 1, D, D, 0.1f, 1.f);
  R(vp + "attn_pool.norm.bias", c->ap_nb, 1, D, D, 0.01f, 0.f);
  R(vp + "attn_pool.mlp.fc1.weight", c->ap_f1w, mlp, D, D, ws, 0.f);
  R(vp + "attn_pool.mlp.fc1.bias", c->ap_f1b, 1, mlp, mlp, 0.01f, 0.f);
  R(vp + "attn_pool.mlp.fc2.weight", c->ap_f2w, D, mlp, mlp, ws, 0.f);
  R(vp + "attn_pool.mlp.fc2.bias", c->ap_f2b, 1, D, D, 0.01f, 0.f);

  // ---- KV cache + activations
  c->kv = P.take<bf16_t>((size_t)L * 2 * c->KVH * T * c->hd);
  c->X = P.take<bf16_t>((size_t)T * d);
  c->Xn = P.take<bf16_t>((size_t)T * d);
  c->QKV = P.take<bf16_t>((size_t)T * qkvn);
  c->Qh = P.take<bf16_t>((size_t)T * d);
  c->AO = P.take<bf16_t>((size_t)T * d);
  c->GU = P.take<bf16_t>((size_t)T * 2 * ff);
  c->ACT = P.take<bf16_t>((size_t)T * ff);
  {
    size_t need = 0;
    const int roles[4][2] = {{qkvn, d}, {d, d}, {2 * ff, d}, {d, ff}};
    for (auto& r : roles) need = std::max(need, (size_t)sk_role_slices(r[0], r[1]) * SK_CHUNK_ROWS * (size_t)r[0]);
    c->skpart_floats = need;
    c->skpart = P.take<float>(need);
  }
  c->ids_dev = P.take<int32_t>(T);
  c->x = P.take<bf16_t>(d);
  c->q = P.take<bf16_t>(d);
  c->act = P.take<bf16_t>(ff);
  c->logits = P.take<float>(V);
  c->pm = P.take<float>((size_t)c->H * 16);          // sized for the largest split factor (dtk_set_option "attn_splits")
  c->pl = P.take<float>((size_t)c->H * 16);
  c->po = P.take<float>((size_t)c->H * 16 * 130);
  c->attn_out = P.take<bf16_t>(d);
  c->attn_ctr = P.take<unsigned>(c->H);
  c->st = P.take<DecState>(1);
  c->sp = P.take<SamplingDev>(1);
  c->smb = P.take<SampleMB>(1);
  c->tok_ring_dev = P.take<int64_t>(DTK_MAX_INFLIGHT);
  c->probs_dev = P.take<float>(V);
  // the tower's activations hold DTK_VIT_BATCH images: dtk_vit_encode(batch) runs them as ONE pass (GEMM rows = images x
  // patches: the M = 729 GEMMs of a single image leave the matrix cores 93 % idle), the prefill uses the first image's share
  const size_t VB = DTK_VIT_BATCH;
  c->pixels_dev = P.take<float>(VB * 3 * c->cfg.vit_image * c->cfg.vit_image);
  c->patches = P.take<bf16_t>(VB * N * c->vPatchLd);
  c->VX = P.take<bf16_t>(VB * N * D);
  c->VN = P.take<bf16_t>(VB * N * D);
  c->VQKV = P.take<bf16_t>(VB * N * 3 * D);
  c->VAO = P.take<bf16_t>(VB * N * D);
  c->VH = P.take<bf16_t>(VB * N * mlp);
  c->feats = P.take<bf16_t>(VB * N * D);
  c->last_hidden = P.take<bf16_t>(VB * N * D);
  c->pq = P.take<bf16_t>(D);
  c->pkv = P.take<bf16_t>(VB * N * 2 * D);
  c->pao = P.take<bf16_t>(VB * D);
  c->px = P.take<bf16_t>(VB * D);
  c->pn = P.take<bf16_t>(VB * D);
  c->ph = P.take<bf16_t>(VB * mlp);
  c->pooled = P.take<bf16_t>(VB * D);
  c->IMG = P.take<bf16_t>((size_t)c->nImg * d);
  if (c->wfmt == 1) {
    for (int i = 0; i < L; ++i) {
      uint8_t* q1 = P.take<uint8_t>((size_t)qkvn * d); float* s1 = P.take<float>(qkvn);
      uint8_t* q2 = P.take<uint8_t>((size_t)d * d);     float* s2 = P.take<float>(d);
      uint8_t* q3 = P.take<uint8_t>((size_t)2 * ff * d); float* s3 = P.take<float>(2 * ff);
      uint8_t* q4 = P.take<uint8_t>((size_t)d * ff);    float* s4 = P.take<float>(d);
      if (reg) {
        LayerW& w = c->layers[i];
        w.q_wqkv = q1; w.s_wqkv = s1; w.q_wo = q2; w.s_wo = s2; w.q_wgu = q3; w.s_wgu = s3; w.q_wdown = q4; w.s_wdown = s4;
      }
    }
    c->q_lm_head = P.take<uint8_t>((size_t)V * d);
    c->s_lm_head = P.take<float>(V);
  }
  if (c->wfmt == 2) {   // MXFP4 layers (codes + block scales, rows padded to whole 32-weight blocks) + the fp8 lm_head
    for (int i = 0; i < L; ++i) {
      uint8_t* q1 = P.take<uint8_t>((size_t)qkvn * mxfp4_row_bytes(d));   uint8_t* s1 = P.take<uint8_t>((size_t)qkvn * mxfp4_row_scales(d));
      uint8_t* q2 = P.take<uint8_t>((size_t)d * mxfp4_row_bytes(d));      uint8_t* s2 = P.take<uint8_t>((size_t)d * mxfp4_row_scales(d));
      uint8_t* q3 = P.take<uint8_t>((size_t)2 * ff * mxfp4_row_bytes(d)); uint8_t* s3 = P.take<uint8_t>((size_t)2 * ff * mxfp4_row_scales(d));
      uint8_t* q4 = P.take<uint8_t>((size_t)d * mxfp4_row_bytes(ff));     uint8_t* s4 = P.take<uint8_t>((size_t)d * mxfp4_row_scales(ff));
      if (reg) {
        LayerW& w = c->layers[i];
        w.f4_wqkv = q1; w.e4_wqkv = s1; w.f4_wo = q2; w.e4_wo = s2; w.f4_wgu = q3; w.e4_wgu = s3; w.f4_wdown = q4; w.e4_wdown = s4;
      }
    }
    c->q_lm_head = P.take<uint8_t>((size_t)V * d);
    c->s_lm_head = P.take<float>(V);
  }
  if (c->nb > 0) {
    c->kv_slot_stride = (size_t)L * 2 * c->KVH * T * 128;
    c->kvb = P.take<bf16_t>((size_t)c->nb * c->kv_slot_stride);
    if (c->kv8) {      // MXFP8 shadow of the decoding slots' decoded rows: 1 + 1/32 bytes per bf16 element of their caches
      c->kv8_slots = c->nb < 16 * c->nt ? c->nb : 16 * c->nt;
      c->kv8c = P.take<uint8_t>((size_t)c->kv8_slots * c->kv_slot_stride);
      c->kv8s = P.take<uint8_t>((size_t)c->kv8_slots * c->kv_slot_stride / 32);
    }
    c->xb = P.take<bf16_t>((size_t)DTK_MAX_BATCH * d);
    // xnb / aob / actb are fragment-major GEMV inputs (common.h xtile_off): K rounded up to whole 32-wide k-steps
    c->xnb = P.take<bf16_t>((size_t)DTK_MAX_BATCH * align_up((size_t)(d > ff ? d : ff), 32));
    c->qb = P.take<bf16_t>((size_t)DTK_MAX_BATCH * d);
    c->aob = P.take<bf16_t>((size_t)DTK_MAX_BATCH * align_up((size_t)d, 32));
    c->actb = P.take<bf16_t>((size_t)DTK_MAX_BATCH * align_up((size_t)ff, 32));
    c->logits_b = P.take<float>((size_t)c->nb * V);
    c->pfx_m = P.take<float>((size_t)DTK_MAX_BATCH * c->H * 4);
    c->pfx_l = P.take<float>((size_t)DTK_MAX_BATCH * c->H * 4);
    c->pfx_o = P.take<float>((size_t)DTK_MAX_BATCH * c->H * 4 * 128);
    c->kpart = P.take<float>((size_t)8 * ((size_t)(d + 15) / 16) * 4 * 256);   // k_gemv_bk: 8 K-slice partials of every row tile x 64 slots
    c->kctr = P.take<unsigned>((size_t)(d + 15) / 16);                              // arrival counters (the arena is zeroed once; the last arrival resets)
    c->st_b = P.take<DecState>(DTK_MAX_SLOTS);
    c->sp_b = P.take<SamplingDev>(DTK_MAX_SLOTS);
    c->smb_b = P.take<SampleMB>(DTK_MAX_SLOTS);
    c->bs_dev = P.take<BatchState>(1);
    if (c->wfmt == 1) {             // fp8: pair-tiled fp8 copies (+6.6 GB for cl-7b), no bf16 tiles
      for (int i = 0; i < L; ++i) {
        uint8_t* a1 = P.take<uint8_t>(tiled_bytes_f8(qkvn, d));
        uint8_t* a2 = P.take<uint8_t>(tiled_bytes_f8(d, d));
        uint8_t* a3 = P.take<uint8_t>(tiled_bytes_f8(2 * ff, d));
        uint8_t* a4 = P.take<uint8_t>(tiled_bytes_f8(d, ff));
        if (reg) { c->layers[i].t8_wqkv = a1; c->layers[i].t8_wo = a2; c->layers[i].t8_wgu = a3; c->layers[i].t8_wdown = a4; }
      }
      c->t8_lm_head = P.take<uint8_t>(tiled_bytes_f8(V, d));
      // (MHA models only: the MXFP8 epilogue of the GQA-fused attention instantiations has not run on hardware yet — a v2 model with fp8
      // weights keeps the bf16-activation kernels)
      c->mx_ok = c->KVH == c->H && mx_unit_covers(d) && mx_kparts_covers(d, d, 32) && mx_kparts_covers(d, ff, 16) && (ff % 64) == 0 && (qkvn % 32) == 0;
      if (c->mx_ok) {               // + one more fp8 copy in MX tile order, the slots' MXFP8 vectors and their scales
        for (int i = 0; i < L; ++i) {
          uint8_t* a1 = P.take<uint8_t>(mx_w_bytes(qkvn, d, 32));
          uint8_t* a2 = P.take<uint8_t>(mx_w_bytes(d, d, 32));
          uint8_t* a3 = P.take<uint8_t>(mx_w_bytes(2 * ff, d, 32));
          uint8_t* a4 = P.take<uint8_t>(mx_w_bytes(d, ff, 16));
          if (reg) { c->layers[i].m_wqkv = a1; c->layers[i].m_wo = a2; c->layers[i].m_wgu = a3; c->layers[i].m_wdown = a4; }
        }
        c->m_lm_head = P.take<uint8_t>(mx_w_bytes(V, d, 32));
        c->xn8 = P.take<uint8_t>(mx_x_bytes(d, 32)); c->xns = P.take<uint8_t>(mx_s_bytes(d, 32));
        c->ao8 = P.take<uint8_t>(mx_x_bytes(d, 32)); c->aos = P.take<uint8_t>(mx_s_bytes(d, 32));
        c->act8 = P.take<uint8_t>(mx_x_bytes(ff, 16)); c->acts = P.take<uint8_t>(mx_s_bytes(ff, 16));
      }
    } else {
      for (int i = 0; i < L; ++i) {   // fragment-major copies of the decoder weights (288 GB HBM: +13 GB for ds-7b)
        bf16_t* a1 = P.take<bf16_t>(tiled_elems(qkvn, d));
        bf16_t* a2 = P.take<bf16_t>(tiled_elems(d, d));
        bf16_t* a3 = P.take<bf16_t>(tiled_elems(2 * ff, d));
        bf16_t* a4 = P.take<bf16_t>(tiled_elems(d, ff));
        if (reg) { c->layers[i].t_wqkv = a1; c->layers[i].t_wo = a2; c->layers[i].t_wgu = a3; c->layers[i].t_wdown = a4; }
      }
      c->t_lm_head = P.take<bf16_t>(tiled_elems(V, d));
    }
    c->tokb_dev = P.take<int64_t>((size_t)DTK_MAX_INFLIGHT * DTK_MAX_BATCH + 1);   // + the sticky device error word (TOKB_ERR)
  }
  for (int i = 0; i < L; ++i) {     // the prefill GEMMs' fragment-major weights: the batched step's copies where a bf16 context has them
    if (sk_role_slices(2 * ff, d) == 1) { bf16_t* ai = P.take<bf16_t>(tiled_elems(2 * ff, d)); if (reg) c->layers[i].p_wgui = ai; }
    if (c->nb > 0 && c->wfmt != 1) { if (reg) { LayerW& w = c->layers[i]; w.p_wqkv = w.t_wqkv; w.p_wo = w.t_wo; w.p_wgu = w.t_wgu; w.p_wdown = w.t_wdown; } continue; }
    bf16_t* a1 = P.take<bf16_t>(tiled_elems(qkvn, d));
    bf16_t* a2 = P.take<bf16_t>(tiled_elems(d, d));
    bf16_t* a3 = P.take<bf16_t>(tiled_elems(2 * ff, d));
    bf16_t* a4 = P.take<bf16_t>(tiled_elems(d, ff));
    if (reg) { LayerW& w = c->layers[i]; w.p_wqkv = a1; w.p_wo = a2; w.p_wgu = a3; w.p_wdown = a4; }
  }
  c->scratch_bytes = (size_t)64 << 20;
  c->scratch = P.take<unsigned char>(c->scratch_bytes);
  c->lp_ring_dev = P.take<float2>(DTK_MAX_INFLIGHT);
  if (c->nb > 0) c->lpb_dev = P.take<float2>((size_t)DTK_MAX_INFLIGHT * DTK_MAX_BATCH);
}

void gemm(dtk_ctx* c, const bf16_t* A, int lda, const bf16_t* W, int ldw, const bf16_t* bias,
          const bf16_t* res, int ldr, bf16_t* C, int ldc, int M, int N, int K, int flags, const bf16_t* gate = nullptr) {
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.residual = res; g.ldr = ldr;
  g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.flags = flags; g.gate = gate;
  hipStream_t s = c->cur_stream ? c->cur_stream : c->stream;
  if (c->gemm_naive) launch_gemm_naive(g, s);
  else launch_gemm_mfma(g, s);
}

// A sliced-K role (g.kslices > 1) at g.M rows: up to SK_SL_MIN_ROWS rows as (tile, slice) blocks + the reduction, in chunks of SK_CHUNK_ROWS
// rows whose partials stay inside the Infinity Cache; above, where the tiles alone fill the chip, as one launch that folds the slices in
// registers.  Same arithmetic per row either way (tested), so a row never depends on how many rows travel with it.
bool gemm_sliced(dtk_ctx* c, const GemmArgs& g, float* part, size_t part_floats, const bf16_t* norm_w, bf16_t* Y, int ldy, hipStream_t s) {
  if (!gemm_sk_supported(g) || (size_t)g.kslices * SK_CHUNK_ROWS * (size_t)g.N > part_floats) return false;
  if (g.M > c->sk_sl_min_rows && launch_gemm_g3_sliced(g, s)) {
    if (norm_w) launch_rmsnorm_rows_sk(g.C, g.ldc, norm_w, Y, ldy, g.M, g.N, c->cfg.rms_eps, s);
    return true;
  }
  for (int m0 = 0; m0 < g.M; m0 += SK_CHUNK_ROWS) {
    GemmArgs h = g;
    h.M = std::min(SK_CHUNK_ROWS, g.M - m0);
    h.A = g.A + (size_t)m0 * g.lda; h.C = g.C + (size_t)m0 * g.ldc; h.residual = g.residual ? g.residual + (size_t)m0 * g.ldr : nullptr;
    h.part = part; h.part_stride = (long)SK_CHUNK_ROWS * g.N;
    if (!launch_gemm_sk(h, norm_w, norm_w ? Y + (size_t)m0 * ldy : nullptr, ldy, c->cfg.rms_eps, s)) return false;
  }
  return true;
}

// One decoder-prefill Linear (+ residual) and, when norm_w is given, the RMSNorm that follows it (-> Y).  Roles whose weight shape gives the
// 256 x 128 tile fewer than 128 blocks run as sliced-K GEMMs (kernels_batched.hip: launch_gemm_sk) — the slice count is a function of the
// WEIGHT shape alone, so a row's arithmetic does not depend on how many rows are prefilled with it (tail prefill == full prefill).
void gemm_role(dtk_ctx* c, const bf16_t* A, int lda, const bf16_t* W, const bf16_t* Wt, int ldw, const bf16_t* res, int ldr, bf16_t* C, int ldc,
               int M, int N, int K, int flags, const bf16_t* norm_w, bf16_t* Y, int ldy) {
  hipStream_t s = c->cur_stream ? c->cur_stream : c->stream;
  const int S = c->prefill_sk ? std::min(sk_role_slices(N, K), c->prefill_sk == 1 ? 8 : c->prefill_sk) : 1;
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = nullptr; g.residual = res; g.ldr = ldr;
  g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.flags = flags; g.kslices = S; g.Wt = Wt;
  bool done = false;
  if (S > 1 && c->gemm_naive) { launch_gemm_naive(g, s); done = true; }
  else if (S > 1) {
    if (!gemm_sliced(c, g, c->skpart, c->skpart_floats, norm_w, Y, ldy, s)) c->launch_refused = true;
    return;
  }    // a sliced role has one canonical order: no silent change of kernel
  if (!done) { g.kslices = 1; if (c->gemm_naive) launch_gemm_naive(g, s); else launch_gemm_mfma(g, s); }
  if (norm_w) launch_rmsnorm_rows(C, ldc, norm_w, Y, ldy, M, N, c->cfg.rms_eps, s);
}

// q/k/v of n <= SK_CHUNK_ROWS prefill rows as a sliced-K GEMM whose reduction is fused with RoPE + the KV append (no [n][qkvn] buffer);
// false = the role is not sliced here (the caller runs Linear + k_rope_scatter).  Same values as that pair, bit for bit.
// rope_rows: the packed scoring pass's {position, cache row} per row instead of start + t for both.
bool qkv_rope_fused(dtk_ctx* c, const LayerW& w, int n, int start, bf16_t* kc, bf16_t* vc, hipStream_t s, const int2* rope_rows = nullptr) {
  const int d = c->d, qkvn = d + 2 * c->KVH * c->hd;
  const int S = c->prefill_sk ? std::min(sk_role_slices(qkvn, d), c->prefill_sk == 1 ? 8 : c->prefill_sk) : 1;
  if (S <= 1 || c->gemm_naive || !c->qkv_rope_fused || n > SK_CHUNK_ROWS || n > c->sk_sl_min_rows || (size_t)S * SK_CHUNK_ROWS * (size_t)qkvn > c->skpart_floats) return false;
  GemmArgs g;
  g.A = c->Xn; g.lda = d; g.W = w.wqkv; g.Wt = w.p_wqkv; g.ldw = d; g.bias = nullptr; g.residual = nullptr; g.ldr = 0;
  g.C = c->QKV; g.ldc = qkvn; g.M = n; g.N = qkvn; g.K = d; g.flags = 0; g.kslices = S;
  g.part = c->skpart; g.part_stride = (long)SK_CHUNK_ROWS * qkvn;
  if (!gemm_sk_supported(g)) return false;
  if (!launch_gemm_sk_partials(g, s)) { c->launch_refused = true; return true; }
  if (rope_rows) launch_sk_rope_scatter_rows(g.part, g.part_stride, S, c->Qh, kc, vc, c->rope_cos, c->rope_sin, n, rope_rows, c->H, c->KVH, c->Tmax, s, c->hd);
  else launch_sk_rope_scatter(g.part, g.part_stride, S, c->Qh, kc, vc, c->rope_cos, c->rope_sin, n, start, c->H, c->KVH, c->Tmax, s, c->hd);
  return true;
}

}  // namespace

int gelu_flag(const dtk_ctx* c) { return c->cfg.vit_gelu_tanh ? GEMM_GELU_TANH : GEMM_GELU_ERF; }

namespace {

bf16_t* kcache(dtk_ctx* c, int layer) { return c->kv + (size_t)layer * 2 * c->KVH * c->Tmax * c->hd; }
bf16_t* vcache(dtk_ctx* c, int layer) { return kcache(c, layer) + (size_t)c->KVH * c->Tmax * c->hd; }

// The adapter's CrossAttentionLayer before ViT block i (reference modeling_adapter.py CrossAttentionLayer.forward) on the B images' rows
// in VX, attending to the cached text.  q_norm is the row LayerNorm over the [rows x heads] x 72 view, in place; the two gated residuals
// are the epilogues of out_proj / fc2 (GEMM_GATED_RESIDUAL).
void cross_layer(dtk_ctx* c, int i, int B, hipStream_t s) {
  const Adapter& A = *c->ad;
  if (!A.present[(size_t)i]) return;
  const CrossW& w = A.layers[(size_t)i];
  const int D = c->vD, N = c->vN, mlp = c->vMlp, Hh = c->vH, hd = c->vHd, R = B * N;
  const float eps = c->cfg.vit_ln_eps;
  launch_layernorm_rows(c->VX, D, w.ln1w, w.ln1b, c->VN, D, R, D, eps, s);
  gemm(c, c->VN, D, w.qw, D, w.qb, nullptr, 0, c->VQKV, D, R, D, D, GEMM_BIAS);
  launch_layernorm_rows(c->VQKV, hd, w.qnw, w.qnb, c->VQKV, hd, R * Hh, hd, eps, s);
  AttnArgs a;
  a.Q = c->VQKV; a.q_sh = hd; a.q_st = D;
  a.K = w.K; a.k_sh = hd; a.k_st = D;
  a.V = w.V; a.v_sh = hd; a.v_st = D;
  a.O = c->VAO; a.o_sh = hd; a.o_st = D;
  a.H = Hh; a.Tq = N; a.Tk = (int)A.text_ids.size(); a.hd = hd; a.causal = 0; a.q_offset = 0; a.scale = 1.0f / sqrtf((float)hd);
  a.impl = c->attn_impl; a.kv_group = 1;
  a.nbatch = B; a.q_sb = (long)N * D; a.k_sb = a.v_sb = 0; a.o_sb = (long)N * D;     // every image attends to the same text
  launch_attention(a, s);
  gemm(c, c->VAO, D, w.ow, D, w.ob, c->VX, D, c->VX, D, R, D, D, GEMM_BIAS | GEMM_RESIDUAL | GEMM_GATED_RESIDUAL, w.gate_a);
  launch_layernorm_rows(c->VX, D, w.ln2w, w.ln2b, c->VN, D, R, D, eps, s);
  gemm(c, c->VN, D, w.f1w, D, w.f1b, nullptr, 0, c->VH, mlp, R, mlp, D, GEMM_BIAS | gelu_flag(c));
  gemm(c, c->VH, mlp, w.f2w, mlp, w.f2b, c->VX, D, c->VX, D, R, D, mlp, GEMM_BIAS | GEMM_RESIDUAL | GEMM_GATED_RESIDUAL, w.gate_m);
}

// ViT trunk + (optionally) MAP head for the image already in pixels_dev; `cross`: with the adapter's layers on the cached text.
void vit_forward(dtk_ctx* c, bool want_pooled, hipStream_t s, int B = 1, bool cross = false) {
  // B images (<= DTK_VIT_BATCH) in one pass: every row-wise op (LayerNorm, the Linear layers) sees B x N rows, attention and the
  // position-embedding add run per image.  Per row the arithmetic is the single-image arithmetic (a GEMM row does not depend on
  // the other rows of its tile), so image b's features are bit-identical to encoding it alone (tested).
  const int D = c->vD, N = c->vN, mlp = c->vMlp, Hh = c->vH, hd = c->vHd;
  const int R = B * N;
  struct StreamScope { dtk_ctx* c; hipStream_t prev; ~StreamScope() { c->cur_stream = prev; } } scope{c, c->cur_stream};
  c->cur_stream = s;
  const size_t img = (size_t)3 * c->cfg.vit_image * c->cfg.vit_image;
  for (int b = 0; b < B; ++b) {
    launch_im2col(c->pixels_dev + (size_t)b * img, c->patches + (size_t)b * N * c->vPatchLd, c->cfg.vit_image, c->cfg.vit_patch, c->vPatchLd, s);
    // conv(patch)+bias -> bf16, then + pos_embed -> bf16 (timm PatchEmbed, _pos_embed): the residual operand is per patch
    gemm(c, c->patches + (size_t)b * N * c->vPatchLd, c->vPatchLd, c->pe_w, c->vPatchLd, c->pe_b, c->pos_embed, D,
         c->VX + (size_t)b * N * D, D, N, D, c->vPatchLd, GEMM_BIAS | GEMM_RESIDUAL);
  }
  const float scale = 1.0f / sqrtf((float)hd);
  const int fl = c->cfg.vit_feature_layer;
  const int last = want_pooled ? c->vDepth - 1 : fl;
  for (int i = 0; i <= last; ++i) {
    const VitBlockW& w = c->vblocks[i];
    if (cross) cross_layer(c, i, B, s);
    launch_layernorm_rows(c->VX, D, w.n1w, w.n1b, c->VN, D, R, D, c->cfg.vit_ln_eps, s);
    gemm(c, c->VN, D, w.qkvw, D, w.qkvb, nullptr, 0, c->VQKV, 3 * D, R, 3 * D, D, GEMM_BIAS);
    {   // the B images' attention problems in ONE launch (grid z = image): 8 launches of 192 blocks each left the chip a quarter empty
      const bf16_t* qkv = c->VQKV;
      AttnArgs a;
      a.Q = qkv; a.q_sh = hd; a.q_st = 3 * D;
      a.K = qkv + D; a.k_sh = hd; a.k_st = 3 * D;
      a.V = qkv + 2 * D; a.v_sh = hd; a.v_st = 3 * D;
      a.O = c->VAO; a.o_sh = hd; a.o_st = D;
      a.H = Hh; a.Tq = N; a.Tk = N; a.hd = hd; a.causal = 0; a.q_offset = 0; a.scale = scale; a.impl = c->attn_impl; a.kv_group = 1;
      a.nbatch = B; a.q_sb = a.k_sb = a.v_sb = (long)N * 3 * D; a.o_sb = (long)N * D;
      launch_attention(a, s);
    }
    gemm(c, c->VAO, D, w.projw, D, w.projb, c->VX, D, c->VX, D, R, D, D, GEMM_BIAS | GEMM_RESIDUAL);
    launch_layernorm_rows(c->VX, D, w.n2w, w.n2b, c->VN, D, R, D, c->cfg.vit_ln_eps, s);
    gemm(c, c->VN, D, w.fc1w, D, w.fc1b, nullptr, 0, c->VH, mlp, R, mlp, D, GEMM_BIAS | gelu_flag(c));
    gemm(c, c->VH, mlp, w.fc2w, mlp, w.fc2b, c->VX, D, c->VX, D, R, D, mlp, GEMM_BIAS | GEMM_RESIDUAL);
    if (i == fl)  // get_intermediate_layers(n=[layer], norm=True)
      launch_layernorm_rows(c->VX, D, c->vnorm_w, c->vnorm_b, c->feats, D, R, D, c->cfg.vit_ln_eps, s);
  }
  if (!want_pooled) return;
  // forward_features -> final norm; forward_head -> AttentionPoolLatent ('map')
  const bf16_t* lh = c->feats;
  if (fl != c->vDepth - 1) {
    launch_layernorm_rows(c->VX, D, c->vnorm_w, c->vnorm_b, c->last_hidden, D, R, D, c->cfg.vit_ln_eps, s);
    lh = c->last_hidden;
  }
  gemm(c, c->ap_latent, D, c->ap_qw, D, c->ap_qb, nullptr, 0, c->pq, D, 1, D, D, GEMM_BIAS);
  gemm(c, lh, D, c->ap_kvw, D, c->ap_kvb, nullptr, 0, c->pkv, 2 * D, R, 2 * D, D, GEMM_BIAS);
  {
    AttnArgs a;
    a.Q = c->pq; a.q_sh = hd; a.q_st = D;
    a.K = c->pkv; a.k_sh = hd; a.k_st = 2 * D;
    a.V = c->pkv + D; a.v_sh = hd; a.v_st = 2 * D;
    a.O = c->pao; a.o_sh = hd; a.o_st = D;
    a.H = Hh; a.Tq = 1; a.Tk = N; a.hd = hd; a.causal = 0; a.q_offset = 0; a.scale = scale; a.impl = c->attn_impl; a.kv_group = 1;
    a.nbatch = B; a.q_sb = 0; a.k_sb = a.v_sb = (long)N * 2 * D; a.o_sb = D;      // the latent query is the same for every image
    launch_attention(a, s);
  }
  gemm(c, c->pao, D, c->ap_pw, D, c->ap_pb, nullptr, 0, c->px, D, B, D, D, GEMM_BIAS);
  launch_layernorm_rows(c->px, D, c->ap_nw, c->ap_nb, c->pn, D, B, D, c->cfg.vit_ln_eps, s);
  gemm(c, c->pn, D, c->ap_f1w, D, c->ap_f1b, nullptr, 0, c->ph, mlp, B, mlp, D, GEMM_BIAS | gelu_flag(c));
  gemm(c, c->ph, mlp, c->ap_f2w, mlp, c->ap_f2b, c->px, D, c->pooled, D, B, D, mlp, GEMM_BIAS | GEMM_RESIDUAL);
}

void project_image(dtk_ctx* c) {
  // feats [N][D] viewed as [N/concat][concat*D] (3 consecutive patch tokens), Linear with bias
  const int K = c->cfg.concat_patches * c->vD;
  gemm(c, c->feats, K, c->mm_w, K, c->proj_bias ? c->mm_b : nullptr, nullptr, 0, c->IMG, c->d, c->nImg, c->d, K,
       c->proj_bias ? GEMM_BIAS : 0);
}

// launches of one decoded token (captured into the graph, or issued directly)
// tokb_dev / tokb_host: the token ring of the batched step + one word the LDS-ring kernels count expired hand-off waits in (it
// travels to the host with every step's tokens; dtk_decode_batch_wait fails once it is non-zero)
#define TOKB_ERR ((size_t)DTK_MAX_INFLIGHT * DTK_MAX_BATCH)
#define TOKB_WORDS (TOKB_ERR + 1)
static inline unsigned* batch_err_word(const dtk_ctx* c) { return reinterpret_cast<unsigned*>(c->tokb_dev + TOKB_ERR); }

#define LPB_BYTES (sizeof(float2) * (size_t)DTK_MAX_INFLIGHT * DTK_MAX_BATCH)
// the D2H copy of the log-probability ring that follows a step's token copy (nothing with the option off)
static inline hipError_t copy_lp_ring(dtk_ctx* c, bool batch) {
  if (!c->logprobs) return hipSuccess;
  if (c->top_logprobs) {
    hipError_t e = batch ? hipMemcpyAsync(c->topb_host, c->topb_dev, sizeof(TopRec) * (size_t)DTK_MAX_INFLIGHT * DTK_MAX_BATCH, hipMemcpyDeviceToHost, c->stream)
                         : hipMemcpyAsync(c->top_ring_host, c->top_ring_dev, sizeof(TopRec) * DTK_MAX_INFLIGHT, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return e;
    e = batch ? hipMemcpyAsync(c->lseb_host, c->lseb_dev, sizeof(float) * (size_t)DTK_MAX_INFLIGHT * DTK_MAX_BATCH, hipMemcpyDeviceToHost, c->stream)
              : hipMemcpyAsync(c->lse_ring_host, c->lse_ring_dev, sizeof(float) * DTK_MAX_INFLIGHT, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return e;
  }
  return batch ? hipMemcpyAsync(c->lpb_host, c->lpb_dev, LPB_BYTES, hipMemcpyDeviceToHost, c->stream)
               : hipMemcpyAsync(c->lp_ring_host, c->lp_ring_dev, sizeof(float2) * DTK_MAX_INFLIGHT, hipMemcpyDeviceToHost, c->stream);
}

// dtk_set_penalties: the PN samplers' view of the step's sequences (nothing without a sequence that has values), and the trailing
// kernel that counts the tokens they sampled
// dtk_set_dry: a step with a sequence that has a multiplier runs the PN samplers too (with 0 / 0 where there is no penalty), k_dry_scan in
// front of them and the trailing kernel, which then also appends to the histories
static void pen_args(const dtk_ctx* c, SampleArgs& sa, DryScanArgs& ds, bool batch) {
  const bool dry = (batch ? c->dry_batch : c->dry_single) && c->dry_tab;
  const bool pen = (batch ? c->pen_batch : c->pen_single) && c->pen_tab;
  // dtk_set_length_control / dtk_set_logit_bias: likewise the PN samplers, which then read the sequences' LenDev records
  const bool len = (batch ? c->len_batch : c->len_single) && c->len_dev;
  if (!(pen || dry || len) || !c->pen_dev || !c->pen_tok) return;
  const int first = batch ? 1 : 0;
  if (len) {
    sa.len = c->len_dev + first; sa.len_m = c->len_m + (size_t)first * c->len_m_stride; sa.len_m_stride = c->len_m_stride;
    sa.bias = c->bias_tab + (size_t)first * c->bias_stride; sa.bias_stride = c->bias_stride;
  }
  // (a launch with DRY alone has records of 0 / 0 and no count tables: nothing reads pen_cnt)
  sa.pen = c->pen_dev + first; sa.pen_cnt = c->pen_tab ? c->pen_tab + (size_t)first * c->pen_stride : nullptr; sa.pen_stride = c->pen_stride;
  sa.pen_tok = c->pen_tok + first;
  if (!dry) return;
  sa.dry = c->dry_dev + first; sa.dry_m = c->dry_tab + (size_t)first * c->dry_stride; sa.dry_stride = c->dry_stride;
  ds.dry = sa.dry; ds.hist = c->dry_hist + (size_t)first * c->Tmax; ds.len = c->dry_len + first; ds.hist_stride = c->Tmax;
  ds.m = c->dry_tab + (size_t)first * c->dry_stride; ds.m_stride = c->dry_stride;
  ds.touched = c->dry_touched + (size_t)first * c->Tmax; ds.n_touched = c->dry_ntouched + first;
  ds.V = sa.V; ds.bs = sa.bs; ds.nslots = sa.bs ? sa.nslots : 1;
}
static void sampler_launch(dtk_ctx* c, SampleArgs& sa, bool mb, bool batch) {
  DryScanArgs ds;
  pen_args(c, sa, ds, batch);
  if (sa.dry) launch_dry_scan(ds, c->stream);
  if (mb) launch_sample_mb(sa, c->stream); else launch_sample_b(sa, c->stream);
  if (sa.pen) launch_count_token(sa, ds, c->stream);
}

// "top_logprobs": the selection in front of the step's sampler, on the logits, DecState and BatchState the sampler is about to read.
// Which kernel: "top_kernel" 1 = k_top_logits, 2 = the sliced pair (kernels_top.hip), 0 = the sliced pair where the row has more than
// one slice (V > 8192) and k_top_logits below, where the pair would be the single block's work in two launches.  Measured at the two
// vocabularies the presets have: the pair is the faster one at V = 128 256 and at V = 32 256, single sequence and 64
// slots (a rule that followed the multi-block sampler, V > 32 768, would leave the v1 vocabularies the slower kernel).  The
// records are the same bits either way.  (top_scratch is allocated with the rings: it is there whenever top_logprobs > 0)
static bool top_use_sliced(const dtk_ctx* c, int V) {
  if (c->top_kernel == 1 || !c->top_scratch || !top_sliced_ok(V, c->top_slice)) return false;
  return c->top_kernel == 2 || V > DTK_TOP_MAX_L;
}
static void top_logits_launch(dtk_ctx* c, const SampleArgs& sa) {
  if (!c->top_logprobs || !c->logprobs) return;
  TopArgs t;
  t.logits = sa.logits; t.V = sa.V; t.logits_stride = sa.logits_stride; t.st = sa.st; t.bs = sa.bs; t.nslots = sa.nslots;
  t.ring = sa.ring; t.k = c->top_logprobs; t.top_ring = sa.bs ? c->topb_dev : c->top_ring_dev;
  if (top_use_sliced(c, sa.V)) { t.L = c->top_slice; t.scratch = c->top_scratch; launch_top_sliced(t, c->stream); }
  else launch_top_logits(t, c->stream);
}

// dtk_set_guidance: the batched step of a context with guided pairs mixes each pair's two pending logits rows into the conditional
// one in front of everything that reads it (guidance_launch), and hands the chosen token to the unconditional slot behind the sampler
// (follow_launch).  A context without a pair: both return at once, the step launches what it launched before
// The pair dimension of the three kernels' grids: the reservation (dtk_reserve_guidance) while the live pairs fit it, else their count
static inline int cfg_grid(const dtk_ctx* c) { return c->cfg_res > c->cfg_n ? c->cfg_res : c->cfg_n; }
static void guidance_launch(dtk_ctx* c, const SampleArgs& sa) {
  if (!cfg_grid(c)) return;
  CfgArgs g;
  g.logits = const_cast<float*>(sa.logits); g.V = sa.V; g.stride = sa.logits_stride; g.pairs = c->cfg_dev; g.n_pairs = cfg_grid(c); g.bs = sa.bs;
  g.part = c->cfg_part; g.lse = c->cfg_lse; g.st = sa.st; g.forced = c->cfg_forced;
  launch_cfg_mix(g, c->stream);
}
static void follow_launch(dtk_ctx* c, const SampleArgs& sa) {
  if (!cfg_grid(c)) return;
  CfgFollowArgs f;
  f.pairs = c->cfg_dev; f.n_pairs = cfg_grid(c); f.bs = sa.bs; f.forced = c->cfg_forced; f.st = sa.st; f.x = sa.x; f.d = sa.d; f.tok_ring = sa.tok_ring; f.ring = sa.ring;
  f.lp_ring = sa.lp_ring; f.lse_ring = sa.lse_ring; f.top_ring = (c->logprobs && c->top_logprobs) ? c->topb_dev : nullptr;
  launch_cfg_follow(f, c->stream);
}

// what a decode step hands its sampler: the single sequence's buffers, or (batch) slot 0's of the batched step over every slot column of
// this step's tiles.  The penalties' tables are bound behind it (pen_args, in sampler_launch)
static SampleArgs step_sample_args(const dtk_ctx* c, bool batch) {
  SampleArgs sa;
  sa.logits = batch ? c->logits_b : c->logits; sa.V = c->V; sa.sp = batch ? c->sp_b : c->sp; sa.st = batch ? c->st_b : c->st; sa.embed = c->embed;
  sa.x = batch ? c->xb : c->x; sa.d = c->d; sa.tok_ring = batch ? c->tokb_dev : c->tok_ring_dev; sa.ring = DTK_MAX_INFLIGHT;
  sa.probs_out = nullptr; sa.advance = 1; sa.step_override = -1;
  sa.bs = batch ? c->bs_dev : nullptr; sa.logits_stride = batch ? c->V : 0; sa.nslots = batch ? 16 * c->nt_step : 1; sa.mb = batch ? c->smb_b : c->smb;
  sa.lp_ring = !c->logprobs ? nullptr : batch ? c->lpb_dev : c->lp_ring_dev;
  sa.trunc = (batch ? c->trunc_batch : c->trunc_single) ? 1 : 0;
  sa.lse_ring = !(c->logprobs && c->top_logprobs) ? nullptr : batch ? c->lseb_dev : c->lse_ring_dev;
  return sa;
}
// the sampling part of a batched step: the guided pairs' mix in front of everything that reads the logits, the top-k records, the sampler,
// the pairs' follower slots behind it (the first and the last: nothing without a guided pair)
static void step_sampler_chain(dtk_ctx* c, SampleArgs& sa, bool mb) {
  guidance_launch(c, sa);
  top_logits_launch(c, sa);
  sampler_launch(c, sa, mb, true);
  follow_launch(c, sa);
}

static inline bool w13_on(const dtk_ctx* c) { return c->wfmt == 0 && c->w13 != 0; }   // the single-sequence step streams 13-bit planes (ensure_w13)

void decode_step_launches(dtk_ctx* c, bool with_probe, bool short_ctx = false) {
  hipStream_t s = c->stream;
  SampleArgs sa = step_sample_args(c, false);
  top_logits_launch(c, sa);
  sampler_launch(c, sa, c->mb_single, false);
  const float scale = 1.0f / sqrtf((float)c->hd);
  for (int l = 0; l < c->L; ++l) {
    const LayerW& w = c->layers[l];
    GemvArgs g{};
    g.eps = c->cfg.rms_eps; g.st = c->st; g.T_max = c->Tmax; g.d = c->d; g.ff = c->ff; g.H = c->H; g.KVH = c->KVH; g.hd = c->hd;
    g.rope_cos = c->rope_cos; g.rope_sin = c->rope_sin;
    g.pm = c->pm; g.pl = c->pl; g.po = c->po; g.S = c->S;
    // 1. input_layernorm + q/k/v projections + RoPE + KV append
    g.W = w.wqkv; g.W8 = w.q_wqkv; g.wscale = w.s_wqkv; g.N = c->d + 2 * c->KVH * c->hd; g.K = c->d; g.x = c->x; g.norm_w = w.ln1;
    g.W4 = w.f4_wqkv; g.S4 = w.e4_wqkv;      // MXFP4 contexts: the four layer roles stream codes + block scales (null otherwise)
    const bool p13 = w13_on(c) && c->w13_ready;   // bf16 contexts: the roles whose matrix has 13-bit planes stream those (same results)
    g.Wp = p13 ? w.p13_wqkv : nullptr; g.Wh = w.h13_wqkv;
    g.q_out = c->q; g.kcache = kcache(c, l); g.vcache = vcache(c, l);
    launch_gemv(PRO_RMSNORM, EPI_QKV, g, s);
    // 2. split-K attention over the cache
    AttnDecArgs ad;
    ad.q = c->q; ad.kcache = kcache(c, l); ad.vcache = vcache(c, l); ad.st = c->st;
    ad.pm = c->pm; ad.pl = c->pl; ad.po = c->po; ad.H = c->H; ad.S = c->S; ad.T_max = c->Tmax; ad.G = c->H / c->KVH;
    ad.scale = scale; ad.hd = c->hd;
    ad.threads = c->attn_threads;
    ad.combine = (!ad.threads && short_ctx && c->attn_combine == 2) ? 3 : c->attn_combine; ad.out = c->attn_out; ad.counters = c->attn_ctr;
    if (ad.threads && ad.combine == 1) ad.combine = 2;      // the tile kernel has no in-kernel combine
    launch_attn_decode(ad, s);
    // 3. (combine +) o_proj + residual
    g.W = w.wo; g.W8 = w.q_wo; g.wscale = w.s_wo; g.N = c->d; g.K = c->d; g.y = c->x;
    g.W4 = w.f4_wo; g.S4 = w.e4_wo;
    g.Wp = p13 ? w.p13_wo : nullptr; g.Wh = w.h13_wo;
    const bool partials = ad.combine == 0 && !(ad.threads && ad.S == 1);   // o_proj's prologue reduces the split partials
    if (!partials) { g.x = c->attn_out; launch_gemv(PRO_COPY, EPI_RESID, g, s); }
    else launch_gemv(PRO_ATTN, EPI_RESID, g, s);
    // 4. post_attention_layernorm + gate/up + SiLU*mul
    g.W = w.wgu; g.W8 = w.q_wgu; g.wscale = w.s_wgu; g.N = 2 * c->ff; g.K = c->d; g.x = c->x; g.norm_w = w.ln2; g.y = c->act;
    g.W4 = w.f4_wgu; g.S4 = w.e4_wgu;
    g.Wp = p13 ? w.p13_wgu : nullptr; g.Wh = w.h13_wgu;
    const bool probe_here = with_probe && (l == c->L / 2);
    if (probe_here) (void)hipEventRecord(c->probe_a, s);
    launch_gemv(PRO_RMSNORM, EPI_SWIGLU, g, s);
    if (probe_here) (void)hipEventRecord(c->probe_b, s);
    // 5. down + residual
    g.W = w.wdown; g.W8 = w.q_wdown; g.wscale = w.s_wdown; g.N = c->d; g.K = c->ff; g.x = c->act; g.y = c->x;
    g.W4 = w.f4_wdown; g.S4 = w.e4_wdown;
    g.Wp = p13 ? w.p13_wdown : nullptr; g.Wh = w.h13_wdown;
    launch_gemv(PRO_COPY, EPI_RESID, g, s);
  }
  GemvArgs g{};      // lm_head: fp8 in an MXFP4 context too (q_lm_head / s_lm_head)
  if (w13_on(c) && c->w13_ready) { g.Wp = c->p13_lm_head; g.Wh = c->h13_lm_head; }
  g.W = c->lm_head; g.W8 = c->q_lm_head; g.wscale = c->s_lm_head; g.N = c->V; g.K = c->d; g.x = c->x; g.norm_w = c->final_norm;
  g.eps = c->cfg.rms_eps; g.logits = c->logits;
  launch_gemv(PRO_RMSNORM, EPI_LOGITS, g, s);
}

static inline bool mx_step(const dtk_ctx* c) { return c->wfmt == 1 && c->mx_ok && c->act_fp8 != 0; }
// kv_format "mxfp8": layer l's shadow planes for the attention of a batched step (a bf16 context: nothing, the bf16 instantiations run)
static inline void kv8_args(const dtk_ctx* c, int l, AttnDecBArgs& ad) {
  if (!c->kv8) return;
  const size_t head_rows = (size_t)c->KVH * c->Tmax, kv_layer = 2 * head_rows * 128;
  ad.k8 = c->kv8c + (size_t)l * kv_layer; ad.v8 = ad.k8 + head_rows * 128;
  ad.k8s = c->kv8s + (size_t)l * (kv_layer / 32); ad.v8s = ad.k8s + head_rows * 4;
  ad.kv8_slot_stride = c->kv_slot_stride;
}

// The MFMA-family step of an fp8 model on the fp8 matrix cores (kernels_batch_mx.hip): 7 launches per layer as the 64-slot bf16
// step — q/k/v, attention, o_proj partials, reduce + residual + RMSNorm, gate/up, down partials, reduce + residual + RMSNorm —
// at every tile count; the vectors between them travel as MXFP8.
void batch_step_launches_mx(dtk_ctx* c) {
  hipStream_t s = c->stream;
  const int d = c->d, ff = c->ff, nslots = 16 * c->nt_step;
  SampleArgs sa = step_sample_args(c, true);
  step_sampler_chain(c, sa, c->mb_batch);
  const float scale = 1.0f / sqrtf(128.f);
  const size_t kv_layer = (size_t)2 * c->KVH * c->Tmax * 128;
  for (int l = 0; l < c->L; ++l) {
    const LayerW& w = c->layers[l];
    bf16_t* kc = c->kvb + (size_t)l * kv_layer;
    bf16_t* vc = kc + (size_t)c->KVH * c->Tmax * 128;
    GemvBArgs g{};
    g.bs = c->bs_dev; g.st = c->st_b; g.T_max = c->Tmax; g.d = d; g.ff = ff; g.H = c->H; g.KVH = c->KVH; g.nt = c->nt_step;
    g.rope_cos = c->rope_cos; g.rope_sin = c->rope_sin; g.kv_slot_stride = c->kv_slot_stride; g.kpart = c->kpart; g.err = batch_err_word(c);
    if (l == 0) launch_rmsnorm_b(c->xb, d, w.ln1, c->xnb, d, d, c->cfg.rms_eps, c->bs_dev, nslots, s, c->xn8, c->xns);
    g.Wm = w.m_wqkv; g.wscale = w.s_wqkv; g.N = d + 2 * c->KVH * 128; g.K = d; g.X8 = c->xn8; g.XS = c->xns; g.q_out = c->qb; g.kcache = kc; g.vcache = vc;
    launch_gemv_mxu(EPI_QKV, g, s);
    AttnDecBArgs ad;
    ad.q = c->qb; ad.kcache = kc; ad.vcache = vc; ad.kv_slot_stride = c->kv_slot_stride; ad.st = c->st_b; ad.bs = c->bs_dev;
    ad.out = c->aob; ad.H = c->H; ad.T_max = c->Tmax; ad.d = d; ad.G = c->H / c->KVH; ad.nslots = nslots;
    ad.scale = scale;
    ad.use_prefix = c->prefix_mfma; ad.pfx_splits = c->pfx_splits; ad.tail_threads = c->tail_threads; ad.gqa_fused = c->gqa_fused; ad.nt_private = c->attn_nt;
    ad.pfx_m = c->pfx_m; ad.pfx_l = c->pfx_l; ad.pfx_o = c->pfx_o;
    ad.out8 = c->ao8; ad.outs = c->aos;
    kv8_args(c, l, ad);
    launch_attn_decode_b(ad, s);
    g.Wm = w.m_wo; g.wscale = w.s_wo; g.N = d; g.K = d; g.X8 = c->ao8; g.XS = c->aos;
    if (!launch_gemv_mxk(g, 32, s)) c->launch_refused = true;
    launch_resid_norm_b(c->kpart, c->xb, d, w.ln2, c->xnb, d, c->cfg.rms_eps, c->bs_dev, nslots, s, c->xn8, c->xns);
    g.Wm = w.m_wgu; g.wscale = w.s_wgu; g.N = 2 * ff; g.K = d; g.X8 = c->xn8; g.XS = c->xns; g.Y8 = c->act8; g.YS = c->acts;
    launch_gemv_mxu(EPI_SWIGLU, g, s);
    g.Wm = w.m_wdown; g.wscale = w.s_wdown; g.N = d; g.K = ff; g.X8 = c->act8; g.XS = c->acts;
    if (!launch_gemv_mxk(g, 16, s)) c->launch_refused = true;
    launch_resid_norm_b(c->kpart, c->xb, d, l + 1 < c->L ? c->layers[l + 1].ln1 : c->final_norm, c->xnb, d, c->cfg.rms_eps, c->bs_dev, nslots, s, c->xn8, c->xns);
  }
  GemvBArgs g{};
  g.bs = c->bs_dev; g.st = c->st_b; g.Wm = c->m_lm_head; g.wscale = c->s_lm_head; g.N = c->V; g.K = d; g.X8 = c->xn8; g.XS = c->xns; g.logits = c->logits_b;
  g.d = d; g.ff = ff; g.nt = c->nt_step; g.H = c->H; g.KVH = c->KVH; g.err = batch_err_word(c);
  launch_gemv_mxu(EPI_LOGITS, g, s);
}

// launches of one batched decode step (all 16 slot columns; inactive slots are skipped in-kernel)
void batch_step_launches(dtk_ctx* c) {
  if (mx_step(c)) { batch_step_launches_mx(c); return; }
  hipStream_t s = c->stream;
  const int d = c->d, ff = c->ff;
  SampleArgs sa = step_sample_args(c, true);
  step_sampler_chain(c, sa, c->mb_batch);
  const float scale = 1.0f / sqrtf(128.f);
  const size_t kv_layer = (size_t)2 * c->KVH * c->Tmax * 128;
  bool kparts = false;
  if (c->resid_kparts) {      // both N = d roles must be covered: the norm placement follows from it for the whole step
    GemvBArgs t{};
    t.nt = c->nt_step; t.kpart = c->kpart; t.W8 = c->layers[0].t8_wo; t.N = d; t.K = d;
    kparts = resid_kparts_covers(t);
    t.K = ff;
    kparts = kparts && resid_kparts_covers(t);
  }
  for (int l = 0; l < c->L; ++l) {
    const LayerW& w = c->layers[l];
    bf16_t* kc = c->kvb + (size_t)l * kv_layer;
    bf16_t* vc = kc + (size_t)c->KVH * c->Tmax * 128;
    GemvBArgs g{};
    g.bs = c->bs_dev; g.st = c->st_b; g.T_max = c->Tmax; g.d = d; g.ff = ff; g.H = c->H; g.KVH = c->KVH; g.nt = c->nt_step;
    g.rope_cos = c->rope_cos; g.rope_sin = c->rope_sin; g.kv_slot_stride = c->kv_slot_stride; g.kpart = c->kpart; g.kctr = c->kctr; g.err = batch_err_word(c);
    // resid_kparts (64 slots): an N = d role is k_gemv_bkp (K split over CUs, fp32 partials stored) and the RMSNorm that follows it
    // is k_resid_norm_b, which first adds the partials + the residual — so the norm of layer l > 0 has already been produced by
    // layer l - 1's down projection, and the final norm by the last layer's
    if (l == 0 || !kparts) launch_rmsnorm_b(c->xb, d, w.ln1, c->xnb, d, d, c->cfg.rms_eps, c->bs_dev, 16 * c->nt_step, s);
    g.W = w.t_wqkv; g.W8 = w.t8_wqkv; g.wscale = w.s_wqkv; g.N = d + 2 * c->KVH * 128; g.K = d; g.X = c->xnb; g.ldx = d; g.q_out = c->qb; g.kcache = kc; g.vcache = vc;
    launch_gemv_b(EPI_QKV, g, s);
    AttnDecBArgs ad;
    ad.q = c->qb; ad.kcache = kc; ad.vcache = vc; ad.kv_slot_stride = c->kv_slot_stride; ad.st = c->st_b; ad.bs = c->bs_dev;
    ad.out = c->aob; ad.H = c->H; ad.T_max = c->Tmax; ad.d = d; ad.G = c->H / c->KVH; ad.nslots = 16 * c->nt_step;
    ad.scale = scale;
    ad.use_prefix = c->prefix_mfma; ad.pfx_splits = c->pfx_splits; ad.tail_threads = c->tail_threads; ad.gqa_fused = c->gqa_fused; ad.nt_private = c->attn_nt;
    ad.pfx_m = c->pfx_m; ad.pfx_l = c->pfx_l; ad.pfx_o = c->pfx_o;
    kv8_args(c, l, ad);
    launch_attn_decode_b(ad, s);
    g.W = w.t_wo; g.W8 = w.t8_wo; g.wscale = w.s_wo; g.N = d; g.K = d; g.X = c->aob; g.ldx = d; g.Y = c->xb; g.ldy = d;
    if (kparts) {
      launch_gemv_bkp(g, s);
      launch_resid_norm_b(c->kpart, c->xb, d, w.ln2, c->xnb, d, c->cfg.rms_eps, c->bs_dev, 16 * c->nt_step, s);
    } else {
      launch_gemv_b(EPI_RESID, g, s);
      launch_rmsnorm_b(c->xb, d, w.ln2, c->xnb, d, d, c->cfg.rms_eps, c->bs_dev, 16 * c->nt_step, s);
    }
    g.W = w.t_wgu; g.W8 = w.t8_wgu; g.wscale = w.s_wgu; g.N = 2 * ff; g.K = d; g.X = c->xnb; g.ldx = d; g.Y = c->actb; g.ldy = ff;
    launch_gemv_b(EPI_SWIGLU, g, s);
    g.W = w.t_wdown; g.W8 = w.t8_wdown; g.wscale = w.s_wdown; g.N = d; g.K = ff; g.X = c->actb; g.ldx = ff; g.Y = c->xb; g.ldy = d;
    if (kparts) {
      launch_gemv_bkp(g, s);
      launch_resid_norm_b(c->kpart, c->xb, d, l + 1 < c->L ? c->layers[l + 1].ln1 : c->final_norm, c->xnb, d, c->cfg.rms_eps, c->bs_dev, 16 * c->nt_step, s);
    } else {
      launch_gemv_b(EPI_RESID, g, s);
    }
  }
  if (!kparts) launch_rmsnorm_b(c->xb, d, c->final_norm, c->xnb, d, d, c->cfg.rms_eps, c->bs_dev, 16 * c->nt_step, s);
  GemvBArgs g{};
  g.bs = c->bs_dev; g.st = c->st_b; g.W = c->t_lm_head; g.W8 = c->t8_lm_head; g.wscale = c->s_lm_head; g.N = c->V; g.K = d; g.X = c->xnb; g.ldx = d; g.logits = c->logits_b;
  g.d = d; g.ff = ff; g.nt = c->nt_step; g.err = batch_err_word(c);
  launch_gemv_b(EPI_LOGITS, g, s);
}

static inline bool mv_family(const dtk_ctx* c) { return c->mv_slots > 0 && c->nb > 0 && c->nb <= c->mv_slots + 1 && c->nb <= 5; }
// slots that may take part in a decode step: 0..3 of a multi-vector context, else the context's column tiles
static inline int max_decode_slots(const dtk_ctx* c) {
  const int lim = mv_family(c) ? 4 : 16 * c->nt;
  return c->nb < lim ? c->nb : lim;
}

// launches of one multi-vector decode step (c->mv_step = 1, 2 or 4 vectors = slots 0..mv_step-1): five kernels per layer
void batch_step_launches_mv(dtk_ctx* c) {
  hipStream_t s = c->stream;
  const int d = c->d, ff = c->ff, NB = c->mv_step;
  // a speculative step (dtk_spec_launch): the same launches over the vectors of ONE sequence — their own DecStates, slot 0's sampling
  // record for every row, the step's own device BatchState, and every vector in slot 0's cache (slot stride 0, no shared-prefix source)
  const bool spec = c->spec_step;
  DecState* const st = spec ? c->spec_st : c->st_b;
  const BatchState* const bs = spec ? c->spec_bs : c->bs_dev;
  const size_t kv_stride = spec ? 0 : c->kv_slot_stride;
  SampleArgs sa = step_sample_args(c, true);
  sa.sp = spec ? c->spec_sp : c->sp_b; sa.st = st; sa.bs = bs; sa.nslots = NB;
  if (spec) {
    // the batched sampler over the pending rows of the vectors that were live in the previous step (dtk_spec_begin refuses a context
    // with penalties, DRY, length rules, a bias, top_logprobs or a guided pair: the plain step's launch is this one), then the two
    // kernels that turn the rows' tokens into the sequence's next tokens and the next step's vectors
    if (c->mb_batch) launch_sample_mb(sa, s); else launch_sample_b(sa, s);
    SpecArgs sv;
    sv.sd = c->spec_sd; sv.hist = c->spec_hist; sv.table = c->spec_table;      // (K, the n-gram size and the draft source are read from spec_sd)
    sv.K = 0; sv.max_ngram = 0; sv.NV = 0; sv.T_max = c->Tmax; sv.V = c->V;
    sv.st_true = c->st_b; sv.st_vec = c->spec_st; sv.bs = c->spec_bs; sv.tok_ring = c->tokb_dev; sv.ring = DTK_MAX_INFLIGHT;
    sv.embed = c->embed; sv.x = c->xb; sv.d = d;
    launch_spec_accept(sv, s);
    if (c->spec_corpus_len > 0) launch_spec_corpus(sv, s);      // (dtk_spec_set_corpus drops the captured steps when this changes)
    launch_spec_draft(sv, s);
  } else {
    step_sampler_chain(c, sa, c->mb_batch);
  }
  const float scale = 1.0f / sqrtf(128.f);
  const size_t kv_layer = (size_t)2 * c->KVH * c->Tmax * 128;
  GemvMvArgs g{};
  g.bs = bs; g.st = st; g.T_max = c->Tmax; g.d = d; g.ff = ff; g.H = c->H; g.KVH = c->KVH; g.eps = c->cfg.rms_eps;
  g.rope_cos = c->rope_cos; g.rope_sin = c->rope_sin; g.kv_slot_stride = kv_stride;
  for (int l = 0; l < c->L; ++l) {
    const LayerW& w = c->layers[l];
    bf16_t* kc = c->kvb + (size_t)l * kv_layer;
    bf16_t* vc = kc + (size_t)c->KVH * c->Tmax * 128;
    // 1. input_layernorm + q/k/v + RoPE + KV append at every slot's own position
    g.W = w.wqkv; g.W8 = w.q_wqkv; g.wscale = w.s_wqkv; g.N = d + 2 * c->KVH * 128; g.K = d; g.X = c->xb; g.ldx = d; g.norm_w = w.ln1;
    g.q_out = c->qb; g.kcache = kc; g.vcache = vc;
    launch_gemv_mv(PRO_RMSNORM, EPI_QKV, NB, g, s);
    // 2. attention: one block per (head, slot), output in fragment order
    AttnDecBArgs ad;
    ad.q = c->qb; ad.kcache = kc; ad.vcache = vc; ad.kv_slot_stride = kv_stride; ad.st = st; ad.bs = bs;
    ad.out = c->aob; ad.H = c->H; ad.T_max = c->Tmax; ad.d = d; ad.G = c->H / c->KVH; ad.nslots = NB;
    ad.scale = scale;
    ad.use_prefix = 0; ad.pfx_splits = c->pfx_splits; ad.tail_threads = c->mv_tail_threads; ad.gqa_fused = c->gqa_fused; ad.nt_private = c->attn_nt;
    ad.pfx_m = c->pfx_m; ad.pfx_l = c->pfx_l; ad.pfx_o = c->pfx_o;
    kv8_args(c, l, ad);
    launch_attn_decode_b(ad, s);
    // 3. o_proj + residual
    g.W = w.wo; g.W8 = w.q_wo; g.wscale = w.s_wo; g.N = d; g.K = d; g.X = c->aob; g.Y = c->xb; g.ldy = d;
    launch_gemv_mv(PRO_COPY, EPI_RESID, NB, g, s);
    // 4. post_attention_layernorm + gate/up + SiLU * mul
    g.W = w.wgu; g.W8 = w.q_wgu; g.wscale = w.s_wgu; g.N = 2 * ff; g.K = d; g.X = c->xb; g.ldx = d; g.norm_w = w.ln2; g.Y = c->actb; g.ldy = ff;
    launch_gemv_mv(PRO_RMSNORM, EPI_SWIGLU, NB, g, s);
    // 5. down + residual
    g.W = w.wdown; g.W8 = w.q_wdown; g.wscale = w.s_wdown; g.N = d; g.K = ff; g.X = c->actb; g.Y = c->xb; g.ldy = d;
    launch_gemv_mv(PRO_COPY, EPI_RESID, NB, g, s);
  }
  g.W = c->lm_head; g.W8 = c->q_lm_head; g.wscale = c->s_lm_head; g.N = c->V; g.K = d; g.X = c->xb; g.ldx = d; g.norm_w = c->final_norm;
  g.logits = c->logits_b;
  launch_gemv_mv(PRO_RMSNORM, EPI_LOGITS, NB, g, s);
}

// fp8 mode: quantise the decoder Linear weights (per-row power-of-two scale) and overwrite the bf16 masters
// with the de-quantised values, so every consumer (prefill GEMM, tiled copy, read-back, oracle) sees the
// same effective weights as the fp8 decode kernels
// MXFP4 mode (wfmt 2): the same for the four layer roles with launch_quant_mxfp4_rows (block scales); lm_head takes the fp8 path
void ensure_fp8_weights(dtk_ctx* c) {
  if (c->wfmt == 0 || c->fp8_ready) return;
  for (int l = 0; l < c->L && c->wfmt == 2; ++l) {
    LayerW& w = c->layers[l];
    launch_quant_mxfp4_rows(w.wqkv, w.f4_wqkv, w.e4_wqkv, c->d + 2 * c->KVH * c->hd, c->d, c->stream);
    launch_quant_mxfp4_rows(w.wo, w.f4_wo, w.e4_wo, c->d, c->d, c->stream);
    launch_quant_mxfp4_rows(w.wgu, w.f4_wgu, w.e4_wgu, 2 * c->ff, c->d, c->stream);
    launch_quant_mxfp4_rows(w.wdown, w.f4_wdown, w.e4_wdown, c->d, c->ff, c->stream);
  }
  for (int l = 0; l < c->L && c->wfmt == 1; ++l) {
    LayerW& w = c->layers[l];
    launch_quant_fp8_rows(w.wqkv, w.q_wqkv, w.s_wqkv, c->d + 2 * c->KVH * c->hd, c->d, c->stream);
    launch_quant_fp8_rows(w.wo, w.q_wo, w.s_wo, c->d, c->d, c->stream);
    launch_quant_fp8_rows(w.wgu, w.q_wgu, w.s_wgu, 2 * c->ff, c->d, c->stream);
    launch_quant_fp8_rows(w.wdown, w.q_wdown, w.s_wdown, c->d, c->ff, c->stream);
  }
  launch_quant_fp8_rows(c->lm_head, c->q_lm_head, c->s_lm_head, c->V, c->d, c->stream);
  c->fp8_ready = true;
  c->tiled_ready = false;
  c->ptiled_ready = false;
}

// accounting: W = decoder layers + final norm + lm_head as the single-sequence step streams them, and the bytes of the
// probe's kernel (gate/up of the middle layer)
static void set_weight_bytes(dtk_ctx* c) {
  const uint64_t kvd = (uint64_t)c->KVH * c->hd;
  const uint64_t attn_lin = (uint64_t)2 * c->d * c->d + 2 * kvd * c->d;   // q, o: d x d; k, v: kvd x d
  const uint64_t per_layer = attn_lin + (uint64_t)3 * c->d * c->ff + 2 * (uint64_t)c->d;
  c->stats.weight_bytes_per_token = 2 * (per_layer * c->L + (uint64_t)c->d + (uint64_t)c->V * c->d);
  if (c->wfmt == 1) {  // 1 byte per Linear weight + fp32 scale per row; norm vectors stay bf16
    const uint64_t lin = attn_lin + (uint64_t)3 * c->d * c->ff;
    const uint64_t rows = (uint64_t)3 * c->d + 2 * kvd + (uint64_t)2 * c->ff;
    c->stats.weight_bytes_per_token = (lin + 4 * rows + 4 * (uint64_t)c->d) * c->L + 2 * (uint64_t)c->d + (uint64_t)c->V * c->d + 4 * (uint64_t)c->V;
  }
  if (c->wfmt == 2) {  // 16 code bytes + 1 scale byte per 32-weight block (rows padded to whole blocks); lm_head fp8 + fp32 row scales; norms bf16
    const uint64_t bd = mxfp4_row_scales(c->d), bf = mxfp4_row_scales(c->ff);
    const uint64_t blocks = ((uint64_t)2 * c->d + 2 * kvd + (uint64_t)2 * c->ff) * bd + (uint64_t)c->d * bf;
    c->stats.weight_bytes_per_token = (17 * blocks + 4 * (uint64_t)c->d) * c->L + 2 * (uint64_t)c->d + (uint64_t)c->V * c->d + 4 * (uint64_t)c->V;
  }
  c->stats.probe_kernel_bytes = (uint64_t)2 * c->ff * c->d * (c->wfmt == 1 ? 1 : 2);
  if (c->wfmt == 2) c->stats.probe_kernel_bytes = (uint64_t)2 * c->ff * 17 * mxfp4_row_scales(c->d);
  if (w13_on(c) && c->w13_ready) {   // planes + the row byte where a matrix has them, bf16 rows where it has not
    auto mat = [](const uint8_t* planes, uint64_t N, int K) { return planes ? N * (w13_row_bytes(K) + 1) : 2 * N * (uint64_t)K; };
    uint64_t W = 2 * ((uint64_t)2 * c->d * c->L + (uint64_t)c->d) + mat(c->p13_lm_head, (uint64_t)c->V, c->d);
    for (int l = 0; l < c->L; ++l) {
      const LayerW& w = c->layers[l];
      W += mat(w.p13_wqkv, (uint64_t)c->d + 2 * kvd, c->d) + mat(w.p13_wo, (uint64_t)c->d, c->d) + mat(w.p13_wgu, (uint64_t)2 * c->ff, c->d) +
           mat(w.p13_wdown, (uint64_t)c->d, c->ff);
    }
    c->stats.weight_bytes_per_token = W;
    c->stats.probe_kernel_bytes = mat(c->layers[c->L / 2].p13_wgu, (uint64_t)2 * c->ff, c->d);
  }
}
static void w13_set_stats(dtk_ctx* c) {
  const uint32_t rows = c->w13_bad_rows > 4095u ? 4095u : c->w13_bad_rows;
  c->stats.w13_counts = (c->w13_packed & 1023u) | ((c->w13_unpacked & 1023u) << 10) | (rows << 20);
}
static int w13_pack_one(dtk_ctx* c, int role, int pro, int epi, const bf16_t* W, int N, int K, uint8_t** planes, uint8_t** hb) {
  GemvArgs g{};
  g.N = N; g.K = K; g.d = c->d; g.ff = c->ff; g.hd = c->hd;
  if (!gemv_w13_takes(pro, epi, g)) {      // the role's bf16 kernel folds in an order no 13-bit shape has (a split-K default): it stays bf16
    if (*planes) { (void)hipFree(*planes); *planes = nullptr; }
    if (*hb) { (void)hipFree(*hb); *hb = nullptr; }
    return DTK_OK;
  }
  if (!*planes) HIPCHK(c, hipMalloc((void**)planes, (size_t)N * w13_row_bytes(K)));
  if (!*hb) HIPCHK(c, hipMalloc((void**)hb, (size_t)N));
  HIPCHK(c, hipMemsetAsync(c->w13_bad, 0, sizeof(unsigned), c->stream));
  launch_pack_w13_rows(W, *planes, *hb, c->w13_bad, N, K, !c->w13_nz, c->stream);
  unsigned bad = 0;
  HIPCHK(c, hipMemcpyAsync(&bad, c->w13_bad, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (bad) {
    (void)hipFree(*planes); *planes = nullptr;
    (void)hipFree(*hb); *hb = nullptr;
    c->w13_unpacked++; c->w13_bad_rows += bad;
  } else {
    c->w13_packed++;
    std::vector<uint8_t> bytes((size_t)N);      // the row bytes: how many rows take the general decode (a figure for the tests and tools)
    HIPCHK(c, hipMemcpy(bytes.data(), *hb, (size_t)N, hipMemcpyDeviceToHost));
    for (uint8_t b : bytes) c->w13_zrows[role] += (b & W13_ZROW) ? 1u : 0u;
  }
  return DTK_OK;
}
static void w13_free(dtk_ctx* c);
// 13-bit planes (w13.h) of the four Linear roles of every layer and of lm_head, for the single-sequence step of a bf16 context with
// option "w13" on.  The bf16 masters are only read: prefill, scoring, the batched and multi-vector steps, read_tensor and the oracle
// see them as before.  A matrix with an unpackable row keeps no planes, and its role then runs the bf16 kernel.  Never inside a capture
// (it allocates and synchronises): the callers run it in front of ensure_graph.  A failure part-way (an allocation) frees every plane, so
// the context is left as with no planes at all and the call can be repeated.
int ensure_w13(dtk_ctx* c) {
  if (!w13_on(c) || c->w13_ready) return DTK_OK;
  if (!c->w13_bad) HIPCHK(c, hipMalloc((void**)&c->w13_bad, sizeof(unsigned)));
  c->w13_packed = c->w13_unpacked = c->w13_bad_rows = 0;
  for (uint32_t& z : c->w13_zrows) z = 0;
  const int qkvn = c->d + 2 * c->KVH * c->hd;
  for (int l = 0; l < c->L; ++l) {
    LayerW& w = c->layers[l];
    int rc = w13_pack_one(c, 0, PRO_RMSNORM, EPI_QKV, w.wqkv, qkvn, c->d, &w.p13_wqkv, &w.h13_wqkv);
    if (!rc) rc = w13_pack_one(c, 1, PRO_ATTN, EPI_RESID, w.wo, c->d, c->d, &w.p13_wo, &w.h13_wo);
    if (!rc) rc = w13_pack_one(c, 2, PRO_RMSNORM, EPI_SWIGLU, w.wgu, 2 * c->ff, c->d, &w.p13_wgu, &w.h13_wgu);
    if (!rc) rc = w13_pack_one(c, 3, PRO_COPY, EPI_RESID, w.wdown, c->d, c->ff, &w.p13_wdown, &w.h13_wdown);
    if (rc) { w13_free(c); return rc; }
  }
  int rc = w13_pack_one(c, 4, PRO_RMSNORM, EPI_LOGITS, c->lm_head, c->V, c->d, &c->p13_lm_head, &c->h13_lm_head);
  if (rc) { w13_free(c); return rc; }
  c->w13_ready = true;
  w13_set_stats(c);
  set_weight_bytes(c);
  return DTK_OK;
}
static void w13_free(dtk_ctx* c) {
  for (auto& w : c->layers) {
    uint8_t** ps[8] = {&w.p13_wqkv, &w.h13_wqkv, &w.p13_wo, &w.h13_wo, &w.p13_wgu, &w.h13_wgu, &w.p13_wdown, &w.h13_wdown};
    for (uint8_t** p : ps) if (*p) { (void)hipFree(*p); *p = nullptr; }
  }
  if (c->p13_lm_head) { (void)hipFree(c->p13_lm_head); c->p13_lm_head = nullptr; }
  if (c->h13_lm_head) { (void)hipFree(c->h13_lm_head); c->h13_lm_head = nullptr; }
  c->w13_ready = false;
  c->w13_packed = c->w13_unpacked = c->w13_bad_rows = 0;
  for (uint32_t& z : c->w13_zrows) z = 0;
}

void ensure_tiled_weights(dtk_ctx* c);
// fragment-major bf16 copies for the prefill GEMMs (of the de-quantised weights in fp8 mode)
void ensure_prefill_tiles(dtk_ctx* c) {
  ensure_fp8_weights(c);
  if (c->ptiled_ready) return;
  for (int l = 0; l < c->L; ++l)
    if (c->layers[l].p_wgui) launch_retile_pairs(c->layers[l].wgu, c->layers[l].p_wgui, c->ff, c->d, c->stream);
  if (c->nb > 0 && c->wfmt != 1) { ensure_tiled_weights(c); c->ptiled_ready = true; return; }
  for (int l = 0; l < c->L; ++l) {
    LayerW& w = c->layers[l];
    launch_retile(w.wqkv, w.p_wqkv, c->d + 2 * c->KVH * c->hd, c->d, c->stream);
    launch_retile(w.wo, w.p_wo, c->d, c->d, c->stream);
    launch_retile(w.wgu, w.p_wgu, 2 * c->ff, c->d, c->stream);
    launch_retile(w.wdown, w.p_wdown, c->d, c->ff, c->stream);
  }
  c->ptiled_ready = true;
}

void ensure_tiled_weights(dtk_ctx* c) {
  ensure_fp8_weights(c);
  if (c->tiled_ready || c->nb <= 0) return;
  if (c->wfmt == 1) {
    const int qkvn = c->d + 2 * c->KVH * 128;
    for (int l = 0; l < c->L; ++l) {
      LayerW& w = c->layers[l];
      launch_retile_f8(w.q_wqkv, w.t8_wqkv, qkvn, c->d, c->stream);
      launch_retile_f8(w.q_wo, w.t8_wo, c->d, c->d, c->stream);
      launch_retile_f8(w.q_wgu, w.t8_wgu, 2 * c->ff, c->d, c->stream);
      launch_retile_f8(w.q_wdown, w.t8_wdown, c->d, c->ff, c->stream);
    }
    launch_retile_f8(c->q_lm_head, c->t8_lm_head, c->V, c->d, c->stream);
    if (c->mx_ok) {
      for (int l = 0; l < c->L; ++l) {
        LayerW& w = c->layers[l];
        launch_retile_mx(w.q_wqkv, w.m_wqkv, qkvn, c->d, 32, c->stream);
        launch_retile_mx(w.q_wo, w.m_wo, c->d, c->d, 32, c->stream);
        launch_retile_mx(w.q_wgu, w.m_wgu, 2 * c->ff, c->d, 32, c->stream);
        launch_retile_mx(w.q_wdown, w.m_wdown, c->d, c->ff, 16, c->stream);
      }
      launch_retile_mx(c->q_lm_head, c->m_lm_head, c->V, c->d, 32, c->stream);
    }
    c->tiled_ready = true;
    return;
  }
  for (int l = 0; l < c->L; ++l) {
    LayerW& w = c->layers[l];
    launch_retile(w.wqkv, w.t_wqkv, c->d + 2 * c->KVH * 128, c->d, c->stream);
    launch_retile(w.wo, w.t_wo, c->d, c->d, c->stream);
    launch_retile(w.wgu, w.t_wgu, 2 * c->ff, c->d, c->stream);
    launch_retile(w.wdown, w.t_wdown, c->d, c->ff, c->stream);
  }
  launch_retile(c->lm_head, c->t_lm_head, c->V, c->d, c->stream);
  c->tiled_ready = true;
}

static inline int nt_index(int nt) { return nt >= 3 ? 2 : nt - 1; }
static inline int step_graph_index(const dtk_ctx* c) { return c->mv_step ? 3 + (c->mv_step >= 4 ? 2 : c->mv_step - 1) : nt_index(c->nt_step); }

void drop_batch_graphs(dtk_ctx* c) {
  for (int i = 0; i < 6; ++i) {
    if (c->bgraph_exec[i]) { (void)hipGraphExecDestroy(c->bgraph_exec[i]); c->bgraph_exec[i] = nullptr; }
    if (c->bgraph[i]) { (void)hipGraphDestroy(c->bgraph[i]); c->bgraph[i] = nullptr; }
    c->bgraph_ready[i] = false;
  }
  for (int i = 0; i < 2; ++i) {      // the speculative steps are captures of the same launches (nothing there without dtk_spec_launch)
    if (c->sgraph_exec[i]) { (void)hipGraphExecDestroy(c->sgraph_exec[i]); c->sgraph_exec[i] = nullptr; }
    if (c->sgraph[i]) { (void)hipGraphDestroy(c->sgraph[i]); c->sgraph[i] = nullptr; }
    c->sgraph_ready[i] = false;
  }
}

void drop_graph(dtk_ctx* c) {          // the single-sequence step's two captures
  if (c->graph_exec) { (void)hipGraphExecDestroy(c->graph_exec); c->graph_exec = nullptr; }
  if (c->graph) { (void)hipGraphDestroy(c->graph); c->graph = nullptr; }
  if (c->graph_short_exec) { (void)hipGraphExecDestroy(c->graph_short_exec); c->graph_short_exec = nullptr; }
  if (c->graph_short) { (void)hipGraphDestroy(c->graph_short); c->graph_short = nullptr; }
  c->graph_ready = false;
}

int ensure_batch_graph(dtk_ctx* c) {   // for c->nt_step / c->mv_step
  const int gi = step_graph_index(c);
  if (c->bgraph_trunc != c->trunc_batch) { drop_batch_graphs(c); c->bgraph_trunc = c->trunc_batch; }
  if (c->bgraph_pen != c->pen_batch) { drop_batch_graphs(c); c->bgraph_pen = c->pen_batch; }
  if (c->bgraph_dry != c->dry_batch) { drop_batch_graphs(c); c->bgraph_dry = c->dry_batch; }
  if (c->bgraph_len != c->len_batch) { drop_batch_graphs(c); c->bgraph_len = c->len_batch; }
  if (c->bgraph_ready[gi]) return DTK_OK;
  HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  c->launch_refused = false;
  if (c->mv_step) batch_step_launches_mv(c); else batch_step_launches(c);
  HIPCHK(c, hipMemcpyAsync(c->tokb_host, c->tokb_dev, sizeof(int64_t) * TOKB_WORDS,
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, copy_lp_ring(c, true));
  HIPCHK(c, hipStreamEndCapture(c->stream, &c->bgraph[gi]));
  if (c->launch_refused || dtk_lds_attr_error(c->device)) {       // an incomplete step must never be replayed
    (void)hipGraphDestroy(c->bgraph[gi]); c->bgraph[gi] = nullptr;
    return fail(c, DTK_ERR_STATE, c->launch_refused ? "batched step: a projection's shape has no kernel in its family (nothing launched for it)"
                                                    : "batched step: raising a kernel's dynamic-LDS limit failed (hipFuncSetAttribute, see stderr)");
  }
  HIPCHK(c, hipGraphInstantiate(&c->bgraph_exec[gi], c->bgraph[gi], nullptr, nullptr, 0));
  c->bgraph_ready[gi] = true;
  c->bgraph_captures++;
  return DTK_OK;
}

int ensure_graph(dtk_ctx* c) {
  if (c->graph_trunc != c->trunc_single) { drop_graph(c); c->graph_trunc = c->trunc_single; }
  if (c->graph_pen != c->pen_single) { drop_graph(c); c->graph_pen = c->pen_single; }
  if (c->graph_dry != c->dry_single) { drop_graph(c); c->graph_dry = c->dry_single; }
  if (c->graph_len != c->len_single) { drop_graph(c); c->graph_len = c->len_single; }
  if (c->graph_ready) return DTK_OK;
  // two captures of the same step: split-K attention (any context) and the one-block-per-head
  // attention used while the context is short; the host picks per step (it knows the position)
  for (int v = 0; v < 2; ++v) {
    HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    decode_step_launches(c, false, v == 1);
    HIPCHK(c, hipMemcpyAsync(c->tok_ring_host, c->tok_ring_dev, sizeof(int64_t) * DTK_MAX_INFLIGHT,
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, copy_lp_ring(c, false));
    HIPCHK(c, hipStreamEndCapture(c->stream, v ? &c->graph_short : &c->graph));
    HIPCHK(c, hipGraphInstantiate(v ? &c->graph_short_exec : &c->graph_exec, v ? c->graph_short : c->graph, nullptr, nullptr, 0));
  }
  c->graph_ready = true;
  return DTK_OK;
}

void compute_rope_tables(const dtk_config& cfg, std::vector<uint16_t>& cosv, std::vector<uint16_t>& sinv) {
  // HF LlamaRotaryEmbedding: inv_freq = 1/theta^(2i/hd) (/factor for 'linear'), fp32;
  // freqs = pos * inv_freq in fp32; cos/sin cast to the activation dtype (bf16).
  const int T = cfg.max_positions, hd = cfg.head_dim, hd2 = hd / 2;
  cosv.resize((size_t)T * hd2); sinv.resize((size_t)T * hd2);
  for (int i = 0; i < hd2; ++i) {
    float inv = (float)(1.0 / pow((double)cfg.rope_theta, (double)(2 * i) / (double)hd));
    if (cfg.rope_factor > 0.f && cfg.rope_factor != 1.f) inv = inv / cfg.rope_factor;
    for (int p = 0; p < T; ++p) {
      const float fr = inv * (float)p;
      cosv[(size_t)p * hd2 + i] = host_f2bf((float)cos((double)fr));
      sinv[(size_t)p * hd2 + i] = host_f2bf((float)sin((double)fr));
    }
  }
}

}  // namespace

// not part of the ABI (hidden): dtk_engine.cpp asks whether its context's steps carry log-probabilities
extern "C" int dtk_internal_logprobs(const dtk_ctx* c) { return (c && c->logprobs) ? 1 : 0; }
// ... likewise "top_logprobs" (k, 0 = off; it cannot be on without "logprobs"): dtk_engine_read_top
extern "C" int dtk_internal_top_logprobs(const dtk_ctx* c) { return (c && c->logprobs) ? c->top_logprobs : 0; }
// ... and tells it how many sequences it holds in the slots (delta = +1 at a join, -1 when the sequence leaves): "logprobs" is refused meanwhile
extern "C" void dtk_internal_engine_holds(dtk_ctx* c, int delta) { if (c) c->engine_holds.fetch_add(delta); }

// ============================================================================ C ABI
// the library is built with -fvisibility=hidden: the C ABI of include/dtk.h is all it exports
#pragma GCC visibility push(default)
extern "C" {

int dtk_abi_version(void) { return DTK_ABI_VERSION; }

// ---- presence / frequency penalties: the count tables -----------------------------------------------------------------------------
static inline int pen_index(const dtk_ctx* c, const SeqHost& sh) { return &sh == &c->seq0 ? 0 : 1 + (int)(&sh - c->bseq.data()); }
static inline bool pen_on(const dtk_ctx* c, int q) { return c->pen_val[q].pp != 0.f || c->pen_val[q].fp != 0.f; }

// everything the feature keeps on the device, at the first non-zero value
// the per-sequence records the PN samplers and the trailing kernel need whatever feature brought them in (penalties or DRY): PenDev
// (0 / 0) and pen_tok (-1).  Each is initialised once, where it is allocated: DRY may have been stepping with them for a while when
// the first penalty arrives
static int pen_alloc_records(dtk_ctx* c) {
  const int nrec = 1 + DTK_MAX_SLOTS;
  if (!c->pen_dev) {
    PenDev* p = nullptr;
    HIPCHK(c, hipMalloc(&p, sizeof(PenDev) * nrec));
    c->pen_dev = p;
    HIPCHK(c, hipMemset(c->pen_dev, 0, sizeof(PenDev) * nrec));
  }
  if (!c->pen_tok) {
    int32_t* p = nullptr;
    HIPCHK(c, hipMalloc(&p, sizeof(int32_t) * nrec));
    c->pen_tok = p;
    HIPCHK(c, hipMemset(c->pen_tok, 0xff, sizeof(int32_t) * nrec));
  }
  if (!c->pen_stage) HIPCHK(c, hipHostMalloc((void**)&c->pen_stage, sizeof(PenDev) * nrec, hipHostMallocDefault));
  return DTK_OK;
}
static int pen_alloc(dtk_ctx* c) {
  if (c->pen_tab) return DTK_OK;
  if (c->Tmax >= 65536) return fail(c, DTK_ERR_RANGE, "penalties: max_positions %d does not fit the 16-bit counts (< 65536)", c->Tmax);
  const int nseq = 1 + c->nb;
  c->pen_stride = (c->V + 7) & ~7;
  // (pen_tab, assigned last, says that everything exists; a buffer that a failed attempt left is kept for the next one and freed with
  // the context)
  if (const int rc = pen_alloc_records(c)) return rc;
  if (!c->pen_ids_dev) HIPCHK(c, hipMalloc(&c->pen_ids_dev, sizeof(int32_t) * (size_t)nseq * c->Tmax));
  if (!c->pen_ids_stage) HIPCHK(c, hipHostMalloc((void**)&c->pen_ids_stage, sizeof(int32_t) * (size_t)nseq * c->Tmax, hipHostMallocDefault));
  uint16_t* tab = nullptr;
  HIPCHK(c, hipMalloc(&tab, sizeof(uint16_t) * (size_t)nseq * c->pen_stride));
  HIPCHK(c, hipMemset(tab, 0, sizeof(uint16_t) * (size_t)nseq * c->pen_stride));
  c->pen_tab = tab;
  return DTK_OK;
}

// Sequence q's table from its token list ids[0, n): zero-fill, then (values != 0 only: a sequence without values keeps an empty table)
// the scatter of ids[start, n).  All on the context's stream from pinned per-sequence staging, so a slot's rebuild queues behind a step
// of the other slots in flight like its sampling upload does.  Nothing before the tables exist.
static int dry_rebuild(dtk_ctx* c, int q, const int64_t* ids, int n, int64_t one_more);
static int pen_rebuild(dtk_ctx* c, int q, const int64_t* ids, int n, int64_t one_more = -1) {
  if (const int rc = dry_rebuild(c, q, ids, n, one_more)) return rc;      // the DRY history is redefined in the same places
  if (!c->pen_tab) return DTK_OK;
  uint16_t* tab = c->pen_tab + (size_t)q * c->pen_stride;
  HIPCHK(c, hipMemsetAsync(tab, 0, sizeof(uint16_t) * (size_t)c->pen_stride, c->stream));
  if (!pen_on(c, q) || !ids) return DTK_OK;
  if (n > c->Tmax) n = c->Tmax;
  int32_t* st = c->pen_ids_stage + (size_t)q * c->Tmax;
  int m = 0;
  for (int i = c->pen_start[q]; i < n; ++i) st[m++] = (int32_t)ids[i];      // (an un-read token, -1, is skipped by the kernel)
  if (one_more >= 0 && n < c->Tmax && c->pen_start[q] <= n) st[m++] = (int32_t)one_more;      // position n: a resumed slot's forced id
  if (m <= 0) return DTK_OK;
  int32_t* dv = c->pen_ids_dev + (size_t)q * c->Tmax;
  HIPCHK(c, hipMemcpyAsync(dv, st, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, c->stream));
  launch_count_scatter(dv, m, tab, c->V, c->stream);
  return DTK_OK;
}

// (extern "C++" here and below: a helper dtk_ops.hip calls too — declared in dtk_ctx.h with C++ linkage and hidden visibility, which the
// definition inside this extern "C" / default-visibility region keeps)
extern "C++" int pen_check(dtk_ctx* c, float pp, float fp, int start, const char* who) {
  if (!(pp >= -2.f && pp <= 2.f)) return fail(c, DTK_ERR_ARG, "%s: presence_penalty must be in [-2, 2]", who);
  if (!(fp >= -2.f && fp <= 2.f)) return fail(c, DTK_ERR_ARG, "%s: frequency_penalty must be in [-2, 2]", who);
  if (start < 0) return fail(c, DTK_ERR_ARG, "%s: penalty_start must be >= 0", who);
  return DTK_OK;
}

// the values of sequence q (0 / 0 / 0: the reset of dtk_set_sampling[_slot]); the table follows them
static int pen_set(dtk_ctx* c, int q, float pp, float fp, int start) {
  const bool on = pp != 0.f || fp != 0.f;
  if (!on && !pen_on(c, q)) { c->pen_start[q] = start; return DTK_OK; }      // nothing to switch off
  if (on) { const int rc = pen_alloc(c); if (rc) return rc; }
  c->pen_val[q].pp = pp; c->pen_val[q].fp = fp; c->pen_start[q] = start;
  c->pen_stage[q] = c->pen_val[q];
  HIPCHK(c, hipMemcpyAsync(c->pen_dev + q, &c->pen_stage[q], sizeof(PenDev), hipMemcpyHostToDevice, c->stream));
  if (q == 0) c->pen_single = on;
  else {
    bool any = false;
    for (int j = 1; j <= c->nb; ++j) any = any || pen_on(c, j);
    c->pen_batch = any;
  }
  const SeqHost& sh = q == 0 ? c->seq0 : c->bseq[(size_t)q - 1];
  return pen_rebuild(c, q, sh.cached_ids.data(), (int)sh.cached_ids.size(), sh.forced_pending);
}

// every table empty: the places that leave the context without any sequence (weights, adapter, options that clear the caches)
static void pen_clear_all(dtk_ctx* c) {
  if (c->pen_tab) (void)hipMemsetAsync(c->pen_tab, 0, sizeof(uint16_t) * (size_t)(1 + c->nb) * c->pen_stride, c->stream);
  if (c->dry_tab) {      // ... and every DRY history
    (void)hipMemsetAsync(c->dry_tab, 0, (size_t)(1 + c->nb) * c->dry_stride, c->stream);
    (void)hipMemsetAsync(c->dry_len, 0, sizeof(DryLen) * (1 + DTK_MAX_SLOTS), c->stream);
    (void)hipMemsetAsync(c->dry_ntouched, 0, sizeof(int32_t) * (1 + DTK_MAX_SLOTS), c->stream);
    for (int q = 0; q <= DTK_MAX_SLOTS; ++q) c->dry_live[q] = c->dry_val[q].on != 0;
  }
}

// ---- DRY: the histories and the match tables -----------------------------------------------------------------------------------------
static inline bool dry_on(const dtk_ctx* c, int q) { return c->dry_val[q].on != 0; }

static int dry_alloc(dtk_ctx* c) {
  if (c->dry_tab) return DTK_OK;
  if (const int rc = pen_alloc_records(c)) return rc;
  const int nseq = 1 + c->nb, nrec = 1 + DTK_MAX_SLOTS;
  c->dry_stride = (c->V + 15) & ~15;
  // (dry_tab, assigned last, says that everything exists, as pen_tab does)
  if (!c->dry_dev) HIPCHK(c, hipMalloc(&c->dry_dev, sizeof(DryDev) * nrec));
  HIPCHK(c, hipMemset(c->dry_dev, 0, sizeof(DryDev) * nrec));
  if (!c->dry_stage) HIPCHK(c, hipHostMalloc((void**)&c->dry_stage, sizeof(DryDev) * nrec, hipHostMallocDefault));
  if (!c->dry_hist) HIPCHK(c, hipMalloc(&c->dry_hist, sizeof(int32_t) * (size_t)nseq * c->Tmax));
  if (!c->dry_hist_stage) HIPCHK(c, hipHostMalloc((void**)&c->dry_hist_stage, sizeof(int32_t) * (size_t)nseq * c->Tmax, hipHostMallocDefault));
  if (!c->dry_len) HIPCHK(c, hipMalloc(&c->dry_len, sizeof(DryLen) * nrec));
  HIPCHK(c, hipMemset(c->dry_len, 0, sizeof(DryLen) * nrec));
  if (!c->dry_len_stage) HIPCHK(c, hipHostMalloc((void**)&c->dry_len_stage, sizeof(DryLen) * nrec, hipHostMallocDefault));
  if (!c->dry_touched) HIPCHK(c, hipMalloc(&c->dry_touched, sizeof(int32_t) * (size_t)nseq * c->Tmax));
  if (!c->dry_ntouched) HIPCHK(c, hipMalloc(&c->dry_ntouched, sizeof(int32_t) * nrec));
  HIPCHK(c, hipMemset(c->dry_ntouched, 0, sizeof(int32_t) * nrec));
  uint8_t* tab = nullptr;
  HIPCHK(c, hipMalloc(&tab, (size_t)nseq * c->dry_stride));
  HIPCHK(c, hipMemset(tab, 0, (size_t)nseq * c->dry_stride));
  c->dry_tab = tab;
  return DTK_OK;
}

// Sequence q's history from its token list ids[0, n) (+ one_more at position n: a resumed slot's forced id): empty table, empty touched
// list, then (multiplier != 0 only) the ids from dry_start on.  On the context's stream from pinned per-sequence staging, as pen_rebuild.
static int dry_rebuild(dtk_ctx* c, int q, const int64_t* ids, int n, int64_t one_more) {
  if (!c->dry_tab) return DTK_OK;
  if (!dry_on(c, q) && !c->dry_live[q]) return DTK_OK;      // never had a multiplier since its last clear: everything is empty already
  c->dry_live[q] = dry_on(c, q);
  HIPCHK(c, hipMemsetAsync(c->dry_tab + (size_t)q * c->dry_stride, 0, (size_t)c->dry_stride, c->stream));
  HIPCHK(c, hipMemsetAsync(c->dry_ntouched + q, 0, sizeof(int32_t), c->stream));
  DryLen& ls = c->dry_len_stage[q];
  ls.n = 0; ls.skip = 0;
  if (dry_on(c, q) && ids) {
    if (n > c->Tmax) n = c->Tmax;
    const int start = c->dry_start[q];
    int32_t* st = c->dry_hist_stage + (size_t)q * c->Tmax;
    int m = 0;
    for (int i = start; i < n; ++i) st[m++] = (int32_t)ids[i];
    int total = n;
    if (one_more >= 0 && n < c->Tmax) { if (start <= n) st[m++] = (int32_t)one_more; total = n + 1; }
    ls.n = m; ls.skip = start > total ? start - total : 0;
    if (m > 0) HIPCHK(c, hipMemcpyAsync(c->dry_hist + (size_t)q * c->Tmax, st, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipMemcpyAsync(c->dry_len + q, &ls, sizeof(DryLen), hipMemcpyHostToDevice, c->stream));
  return DTK_OK;
}

extern "C++" int dry_check(dtk_ctx* c, const dtk_dry* d, int V, const char* who) {
  if (!d) return fail(c, DTK_ERR_ARG, "%s: no dtk_dry", who);
  if (!(d->multiplier >= 0.f && d->multiplier <= 100.f)) return fail(c, DTK_ERR_ARG, "%s: dry_multiplier must be in [0, 100]", who);
  if (!(d->base >= 1.f && d->base <= 8.f)) return fail(c, DTK_ERR_ARG, "%s: dry_base must be in [1, 8]", who);
  if (d->allowed_length < 1 || d->allowed_length > DTK_DRY_MAX_MATCH) return fail(c, DTK_ERR_ARG, "%s: dry_allowed_length must be in [1, %d]", who, DTK_DRY_MAX_MATCH);
  if (d->start < 0) return fail(c, DTK_ERR_ARG, "%s: dry_start must be >= 0", who);
  if (d->n_breakers < 0 || d->n_breakers > DTK_DRY_MAX_BREAKERS) return fail(c, DTK_ERR_ARG, "%s: at most %d dry_sequence_breakers", who, DTK_DRY_MAX_BREAKERS);
  for (int i = 0; i < d->n_breakers; ++i)
    if (d->breakers[i] < 0 || d->breakers[i] >= V) return fail(c, DTK_ERR_ARG, "%s: sequence breaker %d outside [0, %d)", who, d->breakers[i], V);
  return DTK_OK;
}

// the device record of a dtk_dry: pen[L] = 0 below allowed_length, then multiplier * base^(L - allowed_length) by repeated multiplication
// in double, clamped to 1e30 (include/dtk.h: the oracle reproduces it bit for bit)
extern "C++" DryDev dry_record(const dtk_dry* d) {
  DryDev v{};
  if (!d || d->multiplier == 0.f) return v;
  v.on = 1; v.allowed = d->allowed_length; v.n_brk = d->n_breakers;
  for (int i = 0; i < d->n_breakers; ++i) v.brk[i] = d->breakers[i];
  double p = (double)d->multiplier;
  for (int L = d->allowed_length; L <= DTK_DRY_MAX_MATCH; ++L) { v.pen[L] = (float)(p < 1e30 ? p : 1e30); p *= (double)d->base; }
  return v;
}

// the record of sequence q (null / multiplier 0: off, the reset of dtk_set_sampling[_slot]); the history follows it
static int dry_set(dtk_ctx* c, int q, const dtk_dry* d) {
  const bool on = d && d->multiplier != 0.f;
  if (!on && !dry_on(c, q)) { c->dry_start[q] = d ? d->start : 0; return DTK_OK; }      // nothing to switch off
  if (on) { const int rc = dry_alloc(c); if (rc) return rc; }
  c->dry_val[q] = dry_record(d); c->dry_start[q] = d ? d->start : 0;
  c->dry_stage[q] = c->dry_val[q];
  HIPCHK(c, hipMemcpyAsync(c->dry_dev + q, &c->dry_stage[q], sizeof(DryDev), hipMemcpyHostToDevice, c->stream));
  if (q == 0) c->dry_single = on;
  else {
    bool any = false;
    for (int j = 1; j <= c->nb; ++j) any = any || dry_on(c, j);
    c->dry_batch = any;
  }
  const SeqHost& sh = q == 0 ? c->seq0 : c->bseq[(size_t)q - 1];
  return dry_rebuild(c, q, sh.cached_ids.data(), (int)sh.cached_ids.size(), sh.forced_pending);
}

// ---- length control and logit bias: the records, the decay tables and the bias tables ------------------------------------------------
static inline bool len_on(const dtk_ctx* c, int q) { return c->len_val[q].on != 0 || c->len_val[q].n_bias != 0; }

extern "C++" int len_check(dtk_ctx* c, const dtk_length_ctl* l, int V, const char* who) {
  if (!l) return fail(c, DTK_ERR_ARG, "%s: no dtk_length_ctl", who);
  if (l->min_new_tokens < 0) return fail(c, DTK_ERR_ARG, "%s: min_new_tokens must be >= 0", who);
  if (l->decay_start < 0) return fail(c, DTK_ERR_ARG, "%s: decay_start must be >= 0", who);
  if (l->start < 0) return fail(c, DTK_ERR_ARG, "%s: length_start must be >= 0", who);
  if (l->decay_factor != 0.) {
    if (!(l->decay_factor > 0. && l->decay_factor <= DBL_MAX)) return fail(c, DTK_ERR_ARG, "%s: decay_factor must be finite and > 0 (0 = no decay)", who);
    if (l->decay_start < l->min_new_tokens) return fail(c, DTK_ERR_ARG, "%s: decay_start %d is below min_new_tokens %d", who, l->decay_start, l->min_new_tokens);
  }
  if (l->n_eos < 0 || l->n_eos > DTK_LEN_MAX_EOS) return fail(c, DTK_ERR_ARG, "%s: at most %d EOS ids", who, DTK_LEN_MAX_EOS);
  for (int i = 0; i < l->n_eos; ++i)
    if (l->eos_ids[i] < 0 || l->eos_ids[i] >= V) return fail(c, DTK_ERR_ARG, "%s: EOS id %d outside [0, %d)", who, l->eos_ids[i], V);
  return DTK_OK;
}

// the device record of a dtk_length_ctl (null: off); a repeated EOS id is kept once.  n_bias stays with the caller
extern "C++" LenDev len_record(const dtk_length_ctl* l) {
  LenDev v{};
  v.decay_begin = DTK_LEN_NO_DECAY;
  if (!l) return v;
  v.start = l->start; v.min_new = l->min_new_tokens;
  if (l->decay_factor != 0.) v.decay_begin = l->decay_start;
  for (int i = 0; i < l->n_eos; ++i) {
    bool seen = false;
    for (int j = 0; j < v.n_eos; ++j) seen = seen || v.eos[j] == l->eos_ids[i];
    if (!seen) v.eos[v.n_eos++] = l->eos_ids[i];
  }
  v.on = (v.n_eos > 0 && (v.min_new > 0 || v.decay_begin != DTK_LEN_NO_DECAY)) ? 1 : 0;
  return v;
}

// m[k] = min((float)(pow(factor, k) - 1.0), 2^100) for k < n (include/dtk.h: the oracle reproduces it bit for bit)
extern "C++" void len_table(double factor, float* m, int n) {
  for (int k = 0; k < n; ++k) {
    const double v = pow(factor, (double)k) - 1.0;      // (clamped in double: the same value, and no out-of-range conversion)
    m[k] = v < 0x1p100 ? (float)v : 0x1p100f;
  }
}

extern "C++" int bias_check(dtk_ctx* c, const int32_t* ids, const float* values, int n, int V, const char* who) {
  if (n < 0 || n > DTK_BIAS_MAX || (n > 0 && (!ids || !values))) return fail(c, DTK_ERR_ARG, "%s: at most %d (id, value) pairs", who, DTK_BIAS_MAX);
  for (int i = 0; i < n; ++i) {
    if (ids[i] < 0 || ids[i] >= V) return fail(c, DTK_ERR_ARG, "%s: biased id %d outside [0, %d)", who, ids[i], V);
    if (!(values[i] >= -100.f && values[i] <= 100.f)) return fail(c, DTK_ERR_ARG, "%s: a bias must be finite and in [-100, 100]", who);
    for (int j = 0; j < i; ++j)
      if (ids[j] == ids[i]) return fail(c, DTK_ERR_ARG, "%s: id %d is listed twice", who, ids[i]);
  }
  return DTK_OK;
}

// everything the two features keep on the device (with the penalties' records: the rules ride the PN samplers), at the first value that
// is set: the records, the decay tables and the bias tables together, so that a captured step never holds a pointer that is still null
// (len_dev, assigned last, says that everything exists; a buffer that a failed attempt left is kept for the next one)
static int len_alloc_records(dtk_ctx* c) {
  if (c->len_dev) return DTK_OK;
  if (const int rc = pen_alloc_records(c)) return rc;
  const int nrec = 1 + DTK_MAX_SLOTS;
  const size_t nseq = (size_t)(1 + c->nb);
  if (!c->len_stage) HIPCHK(c, hipHostMalloc((void**)&c->len_stage, sizeof(LenDev) * nrec, hipHostMallocDefault));
  c->len_m_stride = c->Tmax + 1;
  if (!c->len_m_stage) HIPCHK(c, hipHostMalloc((void**)&c->len_m_stage, sizeof(float) * nseq * c->len_m_stride, hipHostMallocDefault));
  if (!c->len_m_up) HIPCHK(c, hipEventCreateWithFlags(&c->len_m_up, hipEventDisableTiming));
  if (!c->len_m) {
    float* t = nullptr;
    HIPCHK(c, hipMalloc(&t, sizeof(float) * nseq * c->len_m_stride));
    c->len_m = t;
    HIPCHK(c, hipMemset(c->len_m, 0, sizeof(float) * nseq * c->len_m_stride));
  }
  c->bias_stride = (c->V + 7) & ~7;
  if (!c->bias_tab) {
    float* t = nullptr;
    HIPCHK(c, hipMalloc(&t, sizeof(float) * nseq * c->bias_stride));
    c->bias_tab = t;
    HIPCHK(c, hipMemset(c->bias_tab, 0, sizeof(float) * nseq * c->bias_stride));
  }
  LenDev* p = nullptr;
  HIPCHK(c, hipMalloc(&p, sizeof(LenDev) * nrec));
  for (int q = 0; q < nrec; ++q) c->len_stage[q] = len_record(nullptr);
  if (hipMemcpy(p, c->len_stage, sizeof(LenDev) * nrec, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(p); return fail(c, DTK_ERR_HIP, "length control: the records' upload failed"); }
  c->len_dev = p;
  return DTK_OK;
}
static int len_upload(dtk_ctx* c, int q) {
  c->len_stage[q] = c->len_val[q];
  HIPCHK(c, hipMemcpyAsync(c->len_dev + q, &c->len_stage[q], sizeof(LenDev), hipMemcpyHostToDevice, c->stream));
  if (q == 0) c->len_single = len_on(c, 0);
  else {
    bool any = false;
    for (int j = 1; j <= c->nb; ++j) any = any || len_on(c, j);
    c->len_batch = any;
  }
  return DTK_OK;
}

// the rules of sequence q (null: off, the reset of dtk_set_sampling[_slot]).  The decay table is rebuilt only when the factor changes
static int len_set(dtk_ctx* c, int q, const dtk_length_ctl* l) {
  LenDev v = len_record(l);
  if (!v.on && !c->len_val[q].on) return DTK_OK;      // nothing to switch on or off
  if (const int rc = len_alloc_records(c)) return rc;
  if (v.on && v.decay_begin != DTK_LEN_NO_DECAY) {
    if (c->len_factor[q] != l->decay_factor) {
      HIPCHK(c, hipEventSynchronize(c->len_m_up));      // (the mirror's last upload; done long ago unless two setters follow each other)
      float* st = c->len_m_stage + (size_t)q * c->len_m_stride;
      len_table(l->decay_factor, st, c->len_m_stride);
      HIPCHK(c, hipMemcpyAsync(c->len_m + (size_t)q * c->len_m_stride, st, sizeof(float) * (size_t)c->len_m_stride, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipEventRecord(c->len_m_up, c->stream));
      c->len_factor[q] = l->decay_factor;
    }
  }
  v.n_bias = c->len_val[q].n_bias;
  c->len_val[q] = v;
  return len_upload(c, q);
}

// the bias table of sequence q from n (id, value) pairs (n = 0: none, the reset of dtk_set_sampling[_slot]): the ids the table holds
// go back to 0, then the new pairs are written; pairs whose value is 0 are not kept
static int bias_set(dtk_ctx* c, int q, const int32_t* ids, const float* values, int n) {
  std::vector<int32_t>& held = c->bias_ids[q];
  std::vector<int32_t> nid; std::vector<float> nval;
  for (int i = 0; i < n; ++i) if (values[i] != 0.f) { nid.push_back(ids[i]); nval.push_back(values[i]); }
  if (nid.empty() && held.empty()) return DTK_OK;      // nothing to switch on or off
  if (const int rc = len_alloc_records(c)) return rc;
  float* tab = c->bias_tab + (size_t)q * c->bias_stride;
  launch_bias_scatter(held.data(), nullptr, (int)held.size(), tab, c->V, c->stream);
  launch_bias_scatter(nid.data(), nval.data(), (int)nid.size(), tab, c->V, c->stream);
  HIPCHK(c, hipGetLastError());
  held = nid;
  c->len_val[q].n_bias = (int32_t)nid.size();
  return len_upload(c, q);
}

int dtk_abi_struct_size(int which) {
  switch (which) {
    case 0: return (int)sizeof(dtk_config);
    case 1: return (int)sizeof(dtk_sampling);
    case 2: return (int)sizeof(dtk_stats);
    case 3: return (int)offsetof(dtk_sampling, seed);
    case 4: return (int)offsetof(dtk_config, reserved);
    case 5: return (int)offsetof(dtk_stats, probe_event_pair_ms);
    case 6: return (int)sizeof(dtk_join);
    case 7: return (int)sizeof(dtk_engine_stats);
    case 8: return (int)sizeof(dtk_engine_ops);
    case 9: return (int)offsetof(dtk_join, sampling);
    case 10: return (int)offsetof(dtk_join, error_out);
    case 11: return (int)sizeof(dtk_adapter_config);
    case 12: return (int)sizeof(dtk_sampling_ext);
    case 14: return (int)sizeof(dtk_dry);      // (13 stays unassigned: -1)
    case 16: return (int)sizeof(dtk_length_ctl);      // (15 stays unassigned too)
    case 18: return (int)sizeof(dtk_guided);          // (and 17)
    default: return -1;
  }
}

const char* dtk_last_error(const dtk_ctx* ctx) {
  if (!ctx) return g_create_error.c_str();
  if (g_thread_error_ctx == ctx) return g_thread_error.c_str();     // this thread's own last failure on ctx
  return ctx->err.c_str();
}

int dtk_create(const dtk_config* cfg, int device, dtk_ctx** out) {
  if (!cfg || !out) return fail(nullptr, DTK_ERR_ARG, "dtk_create: null argument");
  *out = nullptr;
  if (cfg->head_dim != 128 && cfg->head_dim != 64) return fail(nullptr, DTK_ERR_ARG, "head_dim must be 128 or 64 (got %d)", cfg->head_dim);
  // head_dim 64 (TinyLlama) has the single-sequence kernels only: the batched-slot step (its q/k/v epilogues, prefix / tail attention,
  // MXFP8 path, kv_fork) is written for 128 — refused here, before anything is allocated or launched
  if (cfg->head_dim == 64 && cfg->reserved[0] > 0)
    return fail(nullptr, DTK_ERR_ARG, "head_dim 64: batched decode slots (batch_slots = %d) have no head_dim-64 kernels yet", cfg->reserved[0]);
  if (cfg->head_dim == 64 && getenv("DTK_ATTN_THREADS") && atoi(getenv("DTK_ATTN_THREADS")) == 0)   // k_attn_decode / _head: hd 128 only
    return fail(nullptr, DTK_ERR_ARG, "DTK_ATTN_THREADS=0: the contiguous-split decode attention has no head_dim-64 kernel (256, 512 or 1024)");
  if (cfg->reserved[1] == 2 && cfg->reserved[0] > 0)   // refused before anything is allocated
    return fail(nullptr, DTK_ERR_ARG, "weight_format mxfp4: MXFP4 weights have no batched-slot or multi-vector kernels yet (batch_slots = %d; use batch_slots = 0)", cfg->reserved[0]);
  if (cfg->reserved[4] != 0 && cfg->reserved[4] != 1)      // key/value row format of decoded tokens: 0 bf16, 1 MXFP8 shadow
    return fail(nullptr, DTK_ERR_ARG, "kv_format %d: 0 (bf16) or 1 (MXFP8 shadow rows for decoded tokens)", cfg->reserved[4]);
  if (cfg->reserved[4] == 1 && cfg->reserved[0] <= 0)
    return fail(nullptr, DTK_ERR_ARG, "kv_format mxfp8: only the batched decode steps read MXFP8 rows (batch_slots = %d; the single-sequence step has no such kernel)", cfg->reserved[0]);
  if (cfg->hidden != cfg->heads * cfg->head_dim)
    return fail(nullptr, DTK_ERR_ARG, "hidden (%d) != heads*head_dim", cfg->hidden);
  if (cfg->reserved[2] < 0 || (cfg->reserved[2] > 0 && cfg->heads % cfg->reserved[2] != 0))
    return fail(nullptr, DTK_ERR_ARG, "kv_heads (%d) must divide heads (%d)", cfg->reserved[2], cfg->heads);
  if (cfg->hidden % 8 || cfg->ffn % 8 || cfg->vit_dim % 8 || cfg->vit_mlp % 8)
    return fail(nullptr, DTK_ERR_ARG, "dims must be multiples of 8");
  if (cfg->vit_dim % cfg->vit_heads) return fail(nullptr, DTK_ERR_ARG, "vit_dim %% vit_heads != 0");
  const int vhd = cfg->vit_dim / cfg->vit_heads;
  if (vhd != 72 && vhd != 128 && vhd != 64 && vhd != 32)
    return fail(nullptr, DTK_ERR_ARG, "unsupported ViT head dim %d", vhd);
  // timm PatchEmbed = Conv2d(stride p): 384/14 -> 27 patches per side, the 6 trailing pixels are dropped
  const int np = cfg->vit_image / cfg->vit_patch;
  if ((np * np) % cfg->concat_patches) return fail(nullptr, DTK_ERR_ARG, "patches %% concat != 0");
  if (cfg->max_positions < 8 || cfg->vocab < 2) return fail(nullptr, DTK_ERR_ARG, "bad sizes");
  if (cfg->vit_feature_layer < 0 || cfg->vit_feature_layer >= cfg->vit_depth)
    return fail(nullptr, DTK_ERR_ARG, "vit_feature_layer out of range");

  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= device)
    return fail(nullptr, DTK_ERR_HIP, "no HIP device %d (count %d: %s)", device, ndev, hipGetErrorString(e));
  dtk_ctx* c = new dtk_ctx();
  c->cfg = *cfg;
  c->device = device;
  c->d = cfg->hidden; c->L = cfg->layers; c->H = cfg->heads; c->ff = cfg->ffn; c->V = cfg->vocab; c->hd = cfg->head_dim;
  c->mb_single = c->mb_batch = sample_mb_supported(cfg->vocab);   // default sampling is greedy: the multi-block chain serves it
  c->KVH = cfg->reserved[2] > 0 ? cfg->reserved[2] : cfg->heads;      // GQA (v2: LLaMA-3.1, 32 / 8)
  c->proj_bias = (cfg->reserved[3] & DTK_ARCH_PROJ_NO_BIAS) == 0;     // v2 connector: Linear(3*D -> d, bias=False)
  c->Tmax = cfg->max_positions;
  // split-K factor of the decode attention: an explicit config value applies to both paths; auto = 16 for one sequence
  // (ds-7b 369.6 -> 373.0, ds-1.3b 1092 -> 1111, v2-8b 343.4 -> 345.1 tok/s over 8) and 8 for the batched step
  // (32 slots already give 8192 blocks: 4.53 ms/step vs 4.69 with 16)
  c->S = cfg->attn_splits > 0 ? cfg->attn_splits : 4;     // tile-interleaved splits: 4 x 128 rows cover 512 keys per memory round trip
  if (const char* es = getenv("DTK_ATTN_SPLITS")) { const int v = atoi(es); if (v >= 1 && v <= 16) c->S = v; }   // tuning aid
  c->wfmt = cfg->reserved[1] == 1 ? 1 : (cfg->reserved[1] == 2 ? 2 : 0);
  // up to 64 decoding slots (one, two or four 16-column MFMA tiles) + up to 8 slots that are only ever prefilled / forked from
  // (prefix cache: one per image in flight, BASELINE config 5 = 8 images)
  c->nb = cfg->reserved[0] < 0 ? 0 : (cfg->reserved[0] > DTK_MAX_SLOTS ? DTK_MAX_SLOTS : cfg->reserved[0]);
  c->nt = c->nb > 33 ? 4 : (c->nb > 17 ? 2 : 1);   // 17 / 33 / 65 = 16 / 32 / 64 decoding slots + the prefix slot
  c->kv8 = cfg->reserved[4] == 1 ? 1 : 0;
  c->bseq.resize((size_t)c->nb);
  c->vD = cfg->vit_dim; c->vDepth = cfg->vit_depth; c->vH = cfg->vit_heads; c->vHd = vhd;
  c->vMlp = cfg->vit_mlp; c->vN = np * np;
  c->vPatchK = 3 * cfg->vit_patch * cfg->vit_patch;
  c->vPatchLd = (int)align_up((size_t)c->vPatchK, 8);
  c->nImg = c->vN / cfg->concat_patches;
  const char* gm = getenv("DTK_GEMM");
  c->gemm_naive = gm && !strcmp(gm, "naive");
  const char* ac = getenv("DTK_ATTN_COMBINE");
  // measured default (tools/tune_decode.py, profiles/r02_tune_decode_*.log): 512-thread tile kernel, 4 splits, partials reduced in
  // o_proj's prologue — one launch less per layer (ds-7b 384.2 -> 387.0 tok/s, ds-1.3b 1137 -> 1174)
  c->attn_combine = !ac ? 0 : (!strcmp(ac, "consumer") ? 0 : (!strcmp(ac, "inkernel") ? 1 : 2));
  c->attn_threads = 512;
  if (const char* at = getenv("DTK_ATTN_THREADS")) c->attn_threads = atoi(at);

  if (c->S > 16) c->S = 16;
  if (const char* fm = getenv("DTK_ATTN_FULL_MAX")) c->attn_full_max = atoi(fm);
  if (const char* gv = getenv("DTK_GEMV_VARIANTS")) {  // "epi:variant,epi:variant" (tuning aid)
    int e = 0, v = 0;
    const char* p = gv;
    while (sscanf(p, "%d:%d", &e, &v) == 2) {
      set_gemv_default_variant(e, v);
      p = strchr(p, ',');
      if (!p) break;
      ++p;
    }
  }

#define CCHK(call)                                                                         \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess) {                                                                \
      fail(nullptr, DTK_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_));           \
      dtk_destroy(c);                                                                      \
      return DTK_ERR_HIP;                                                                  \
    }                                                                                      \
  } while (0)
  CCHK(hipSetDevice(device));
  CCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  CCHK(hipStreamCreateWithFlags(&c->stream_vit, hipStreamNonBlocking));
  Planner sz;
  plan(c, sz, false);
  c->arena_bytes = align_up(sz.off, 256) + 256;
  CCHK(hipMalloc((void**)&c->arena, c->arena_bytes));
  Planner real;
  real.base = c->arena;
  plan(c, real, true);
  CCHK(hipMemsetAsync(c->arena, 0, c->arena_bytes, c->stream));
  if (c->kv8) {      // a shadow row read before it was written is NaN, as a code and as a scale
    CCHK(hipMemsetAsync(c->kv8c, 0xFF, (size_t)c->kv8_slots * c->kv_slot_stride, c->stream));
    CCHK(hipMemsetAsync(c->kv8s, 0xFF, (size_t)c->kv8_slots * c->kv_slot_stride / 32, c->stream));
  }
  CCHK(hipHostMalloc((void**)&c->tok_ring_host, sizeof(int64_t) * DTK_MAX_INFLIGHT, hipHostMallocDefault));
  CCHK(hipHostMalloc((void**)&c->lp_ring_host, sizeof(float2) * DTK_MAX_INFLIGHT, hipHostMallocDefault));
  for (int i = 0; i < DTK_MAX_INFLIGHT; ++i) CCHK(hipEventCreateWithFlags(&c->step_done[i], hipEventDisableTiming));
  if (c->nb > 0) {
    CCHK(hipHostMalloc((void**)&c->bs_host, sizeof(BatchState) * DTK_MAX_INFLIGHT, hipHostMallocDefault));
    CCHK(hipHostMalloc((void**)&c->tokb_host, sizeof(int64_t) * TOKB_WORDS, hipHostMallocDefault));
    CCHK(hipHostMalloc((void**)&c->lpb_host, LPB_BYTES, hipHostMallocDefault));
    CCHK(hipHostMalloc((void**)&c->st_stage, sizeof(DecState) * (DTK_MAX_SLOTS), hipHostMallocDefault));
    CCHK(hipHostMalloc((void**)&c->sp_stage, sizeof(SamplingDev) * (DTK_MAX_SLOTS), hipHostMallocDefault));
    CCHK(hipHostMalloc((void**)&c->draw_stage, sizeof(uint32_t) * (DTK_MAX_SLOTS), hipHostMallocDefault));
    for (int i = 0; i < DTK_MAX_INFLIGHT; ++i) CCHK(hipEventCreateWithFlags(&c->bstep_done[i], hipEventDisableTiming));
  }
  CCHK(hipEventCreate(&c->ev_a)); CCHK(hipEventCreate(&c->ev_b)); CCHK(hipEventCreate(&c->ev_c));
  CCHK(hipEventCreate(&c->ev_va)); CCHK(hipEventCreate(&c->ev_vb));
  CCHK(hipEventCreate(&c->probe_a)); CCHK(hipEventCreate(&c->probe_b));
  // default RoPE tables (the Python loader overrides them with torch-computed ones)
  std::vector<uint16_t> cosv, sinv;
  compute_rope_tables(*cfg, cosv, sinv);
  CCHK(hipMemcpyAsync(c->rope_cos, cosv.data(), cosv.size() * 2, hipMemcpyHostToDevice, c->stream));
  CCHK(hipMemcpyAsync(c->rope_sin, sinv.data(), sinv.size() * 2, hipMemcpyHostToDevice, c->stream));
  CCHK(hipStreamSynchronize(c->stream));
#undef CCHK
  // accounting: W = decoder layers + final norm + lm_head, K = 2*L*d*2
  set_weight_bytes(c);
  c->stats.kv_bytes_per_ctx_token = (uint64_t)2 * c->L * (uint64_t)c->KVH * c->hd * 2;
  *out = c;
  // Batched attention shape, a property of the CONTEXT (like the multi-vector family): 64 decoding slots -> shared prefixes on the
  // matrix cores + 2-wave tail blocks; fewer -> the per-slot walk with 4-wave blocks.  Measured over a rollout's private lengths
  // (profiles/r05g_step_bench.txt, ds-7b, ms per step at 4 / 260 / 480 private keys): 64 slots 3.96 / 5.43 / 6.52 against 4.35 / 5.67 /
  // 6.57 for round 4's shape; 16 slots 3.31 / 3.99 / 4.40 against 3.45 / 3.69 / 3.94 — with 512 blocks the prefix kernel's launch is not
  // paid back and 2-wave blocks keep too few loads in flight.  A slot's arithmetic depends on its context's size, never on the active set.
  if (c->nb > 0) {
    const bool big = max_decode_slots(c) >= 64;
    c->prefix_mfma = big ? 1 : 0;
    c->tail_threads = big ? 128 : 256;
  }
  if (const char* opts = getenv("DTK_OPTIONS")) {   // "name=value,name=value": dtk_set_option at create (profiling runs of unmodified tools)
    std::string all(opts);
    size_t at = 0;
    while (at < all.size()) {
      size_t end = all.find(',', at);
      if (end == std::string::npos) end = all.size();
      const std::string item = all.substr(at, end - at);
      const size_t eq = item.find('=');
      if (eq != std::string::npos && dtk_set_option(c, item.substr(0, eq).c_str(), atoi(item.c_str() + eq + 1)) != DTK_OK)
        fprintf(stderr, "DTK_OPTIONS: %s rejected (%s)\n", item.c_str(), c->err.c_str());
      at = end + 1;
    }
  }
  return DTK_OK;
}

void dtk_destroy(dtk_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->ad) (void)dtk_adapter_destroy(c);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  w13_free(c);
  if (c->w13_bad) (void)hipFree(c->w13_bad);
  if (c->graph_exec) (void)hipGraphExecDestroy(c->graph_exec);
  if (c->graph) (void)hipGraphDestroy(c->graph);
  if (c->graph_short_exec) (void)hipGraphExecDestroy(c->graph_short_exec);
  if (c->graph_short) (void)hipGraphDestroy(c->graph_short);
  drop_batch_graphs(c);
  for (int i = 0; i < DTK_MAX_INFLIGHT; ++i) if (c->bstep_done[i]) (void)hipEventDestroy(c->bstep_done[i]);
  if (c->bs_host) (void)hipHostFree(c->bs_host);
  if (c->tokb_host) (void)hipHostFree(c->tokb_host);
  if (c->lpb_host) (void)hipHostFree(c->lpb_host);
  if (c->lp_ring_host) (void)hipHostFree(c->lp_ring_host);
  if (c->st_stage) (void)hipHostFree(c->st_stage);
  if (c->sp_stage) (void)hipHostFree(c->sp_stage);
  if (c->draw_stage) (void)hipHostFree(c->draw_stage);
  for (int i = 0; i < DTK_MAX_INFLIGHT; ++i) if (c->step_done[i]) (void)hipEventDestroy(c->step_done[i]);
  hipEvent_t evs[] = {c->ev_a, c->ev_b, c->ev_c, c->probe_a, c->probe_b};
  for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e);
  if (c->tok_ring_host) (void)hipHostFree(c->tok_ring_host);
  if (c->arena) (void)hipFree(c->arena);
  if (c->score_rec) (void)hipFree(c->score_rec);
  if (c->score_out) (void)hipFree(c->score_out);
  if (c->score_top) (void)hipFree(c->score_top);
  if (c->pen_tab) (void)hipFree(c->pen_tab);
  if (c->pen_dev) (void)hipFree(c->pen_dev);
  if (c->pen_tok) (void)hipFree(c->pen_tok);
  if (c->pen_ids_dev) (void)hipFree(c->pen_ids_dev);
  if (c->pen_ids_stage) (void)hipHostFree(c->pen_ids_stage);
  if (c->pen_stage) (void)hipHostFree(c->pen_stage);
  if (c->dry_tab) (void)hipFree(c->dry_tab);
  if (c->dry_dev) (void)hipFree(c->dry_dev);
  if (c->dry_stage) (void)hipHostFree(c->dry_stage);
  if (c->dry_hist) (void)hipFree(c->dry_hist);
  if (c->dry_hist_stage) (void)hipHostFree(c->dry_hist_stage);
  if (c->dry_len) (void)hipFree(c->dry_len);
  if (c->dry_len_stage) (void)hipHostFree(c->dry_len_stage);
  if (c->dry_touched) (void)hipFree(c->dry_touched);
  if (c->dry_ntouched) (void)hipFree(c->dry_ntouched);
  if (c->len_dev) (void)hipFree(c->len_dev);
  if (c->len_stage) (void)hipHostFree(c->len_stage);
  if (c->len_m) (void)hipFree(c->len_m);
  if (c->len_m_stage) (void)hipHostFree(c->len_m_stage);
  if (c->bias_tab) (void)hipFree(c->bias_tab);
  if (c->len_m_up) (void)hipEventDestroy(c->len_m_up);
  if (c->top_ring_dev) (void)hipFree(c->top_ring_dev);
  if (c->lse_ring_dev) (void)hipFree(c->lse_ring_dev);
  if (c->topb_dev) (void)hipFree(c->topb_dev);
  if (c->lseb_dev) (void)hipFree(c->lseb_dev);
  if (c->top_scratch) (void)hipFree(c->top_scratch);
  if (c->cfg_dev) (void)hipFree(c->cfg_dev);
  if (c->cfg_part) (void)hipFree(c->cfg_part);
  if (c->cfg_lse) (void)hipFree(c->cfg_lse);
  if (c->cfg_forced) (void)hipFree(c->cfg_forced);
  if (c->top_ring_host) (void)hipHostFree(c->top_ring_host);
  if (c->lse_ring_host) (void)hipHostFree(c->lse_ring_host);
  if (c->topb_host) (void)hipHostFree(c->topb_host);
  if (c->lseb_host) (void)hipHostFree(c->lseb_host);
  if (c->packed_rows) (void)hipFree(c->packed_rows);
  if (c->spec_mem) (void)hipFree(c->spec_mem);
  if (c->spec_corpus) (void)hipFree(c->spec_corpus);
  if (c->stream_vit) (void)hipStreamDestroy(c->stream_vit);
  if (c->ev_va) (void)hipEventDestroy(c->ev_va);
  if (c->ev_vb) (void)hipEventDestroy(c->ev_vb);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int dtk_num_tensors(const dtk_ctx* c) { return c ? (int)c->tensors.size() : 0; }
const char* dtk_tensor_name(const dtk_ctx* c, int i) {
  if (!c || i < 0 || i >= (int)c->tensors.size()) return nullptr;
  return c->tensors[i].name.c_str();
}
int64_t dtk_tensor_numel(const dtk_ctx* c, const char* name) {
  if (!c || !name) return -1;
  auto it = c->tindex.find(name);
  return it == c->tindex.end() ? -1 : c->tensors[it->second].numel();
}

int dtk_load_tensor(dtk_ctx* c, const char* name, const void* host, int dtype, const int64_t* shape, int ndim) {
  if (!c || !name || !host || !shape || ndim < 1) return fail(c, DTK_ERR_ARG, "dtk_load_tensor: null argument");
  auto it = c->tindex.find(name);
  if (it == c->tindex.end()) return fail(c, DTK_ERR_ARG, "unknown tensor '%s'", name);
  TensorEntry& t = c->tensors[it->second];
  int64_t n = 1;
  for (int i = 0; i < ndim; ++i) n *= shape[i];
  if (n != t.numel()) return fail(c, DTK_ERR_ARG, "tensor '%s': %lld elements given, %lld expected", name, (long long)n, (long long)t.numel());
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<uint16_t> tmp;
  const uint16_t* src16 = nullptr;
  if (dtype == DTK_BF16) {
    src16 = static_cast<const uint16_t*>(host);
  } else if (dtype == DTK_F32) {
    tmp.resize((size_t)n);
    const float* f = static_cast<const float*>(host);
    for (int64_t i = 0; i < n; ++i) tmp[(size_t)i] = host_f2bf(f[i]);
    src16 = tmp.data();
  } else if (dtype == DTK_F16) {
    tmp.resize((size_t)n);
    const uint16_t* hf = static_cast<const uint16_t*>(host);
    for (int64_t i = 0; i < n; ++i) tmp[(size_t)i] = host_f2bf(host_h2f(hf[i]));
    src16 = tmp.data();
  } else {
    return fail(c, DTK_ERR_ARG, "bad dtype %d", dtype);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy2D(t.ptr, (size_t)t.stride * 2, src16, (size_t)t.cols * 2, (size_t)t.cols * 2, (size_t)t.rows, hipMemcpyHostToDevice));
  t.loaded = true;
  if (c->ad) { c->ad->text_ids.clear(); c->ad->dummy_host.clear(); c->ad->emb->ptiled_ready = false; }
  c->have_image = false;
  c->seq0.cached_ids.clear();
  for (auto& b : c->bseq) b.cached_ids.clear();
  pen_clear_all(c);
  c->tiled_ready = false;
  c->ptiled_ready = false;
  c->fp8_ready = false;
  if (c->w13_ready) { c->w13_ready = false; drop_graph(c); set_weight_bytes(c); }   // the planes are packed again before the next single-sequence step
  return DTK_OK;
}

int dtk_read_tensor(dtk_ctx* c, const char* name, void* host_out, int64_t n_elems) {
  if (!c || !name || !host_out) return fail(c, DTK_ERR_ARG, "dtk_read_tensor: null argument");
  auto it = c->tindex.find(name);
  if (it == c->tindex.end()) return fail(c, DTK_ERR_ARG, "unknown tensor '%s'", name);
  const TensorEntry& t = c->tensors[it->second];
  if (n_elems != t.numel()) return fail(c, DTK_ERR_ARG, "tensor '%s' has %lld elements", name, (long long)t.numel());
  HIPCHK(c, hipSetDevice(c->device));
  ensure_fp8_weights(c);   // fp8 mode: the stored tensor is the de-quantised (effective) weight
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy2D(host_out, (size_t)t.cols * 2, t.ptr, (size_t)t.stride * 2, (size_t)t.cols * 2, (size_t)t.rows, hipMemcpyDeviceToHost));
  return DTK_OK;
}

int dtk_fill_synthetic(dtk_ctx* c, uint64_t seed) {
  if (!c) return DTK_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  for (size_t i = 0; i < c->tensors.size(); ++i) {
    TensorEntry& t = c->tensors[i];
    if (t.name == "rope.cos" || t.name == "rope.sin" || t.name == "embedding_model.rope.cos" || t.name == "embedding_model.rope.sin") continue;
    t.loaded = true;
    if (t.stride == t.cols) {
      launch_fill_synth(t.ptr, t.numel(), seed, (uint32_t)i, t.synth_scale, t.synth_offset, c->stream);
    } else {  // padded rows: fill contiguously in scratch, then pitch-copy
      if ((size_t)t.numel() * 2 > c->scratch_bytes) return fail(c, DTK_ERR_ARG, "scratch too small");
      bf16_t* tmp = reinterpret_cast<bf16_t*>(c->scratch);
      launch_fill_synth(tmp, t.numel(), seed, (uint32_t)i, t.synth_scale, t.synth_offset, c->stream);
      HIPCHK(c, hipMemcpy2DAsync(t.ptr, (size_t)t.stride * 2, tmp, (size_t)t.cols * 2, (size_t)t.cols * 2, (size_t)t.rows, hipMemcpyDeviceToDevice, c->stream));
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->ad) { c->ad->text_ids.clear(); c->ad->dummy_host.clear(); c->ad->emb->ptiled_ready = false; }
  c->have_image = false;
  c->seq0.cached_ids.clear();
  for (auto& b : c->bseq) b.cached_ids.clear();
  pen_clear_all(c);
  c->tiled_ready = false;
  c->ptiled_ready = false;
  c->fp8_ready = false;
  if (c->w13_ready) { c->w13_ready = false; drop_graph(c); set_weight_bytes(c); }   // the planes are packed again before the next single-sequence step
  return DTK_OK;
}

static int vit_encode_impl(dtk_ctx* c, const float* pixels, int batch, void* feats_out, void* pooled_out, const int64_t* text_ids, int T_text);
static int text_prepare(dtk_ctx* c, const int64_t* ids, int T, hipStream_t s);
int dtk_vit_encode(dtk_ctx* c, const float* pixels, int batch, void* feats_out, void* pooled_out) {
  return vit_encode_impl(c, pixels, batch, feats_out, pooled_out, nullptr, 0);
}

static int vit_encode_impl(dtk_ctx* c, const float* pixels, int batch, void* feats_out, void* pooled_out, const int64_t* text_ids, int T_text) {
  if (!c || !pixels || batch < 1) return fail(c, DTK_ERR_ARG, "dtk_vit_encode: bad argument");
  if (pooled_out) {   // forward_head needs the attention-pool weights: a checkpoint without them must not pool with zeros
    for (const TensorEntry& t : c->tensors)
      if (!t.loaded && t.name.compare(0, 23, "vision_model.attn_pool.") == 0)
        return fail(c, DTK_ERR_STATE, "pooler_output requested but '%s' was never loaded (checkpoint without the pooling head)", t.name.c_str());
  }
  std::lock_guard<std::mutex> vit_guard(c->vit_mu);
  HIPCHK(c, hipSetDevice(c->device));
  const size_t img = (size_t)3 * c->cfg.vit_image * c->cfg.vit_image;
  hipStream_t sv = c->stream_vit;
  // forward() semantics (pooled requested): last_hidden_state = forward_features = ALL blocks + final norm; without the
  // head: get_intermediate_layers(n=[feature_layer], norm=True).  The two differ when feature_layer != depth - 1.
  const bf16_t* hidden = (pooled_out && c->cfg.vit_feature_layer != c->vDepth - 1) ? c->last_hidden : c->feats;
  if (text_ids) { const int rc = text_prepare(c, text_ids, T_text, sv); if (rc != DTK_OK) return rc; }
  for (int b0 = 0; b0 < batch; b0 += DTK_VIT_BATCH) {
    const int B = std::min(batch - b0, (int)DTK_VIT_BATCH);
    HIPCHK(c, hipMemcpyAsync(c->pixels_dev, pixels + (size_t)b0 * img, (size_t)B * img * 4, hipMemcpyHostToDevice, sv));
    HIPCHK(c, hipEventRecord(c->ev_va, sv));
    vit_forward(c, pooled_out != nullptr, sv, B, text_ids != nullptr);
    HIPCHK(c, hipEventRecord(c->ev_vb, sv));
    if (feats_out)
      HIPCHK(c, hipMemcpyAsync((bf16_t*)feats_out + (size_t)b0 * c->vN * c->vD, hidden, (size_t)B * c->vN * c->vD * 2, hipMemcpyDeviceToHost, sv));
    if (pooled_out)
      HIPCHK(c, hipMemcpyAsync((bf16_t*)pooled_out + (size_t)b0 * c->vD, c->pooled, (size_t)B * c->vD * 2, hipMemcpyDeviceToHost, sv));
    HIPCHK(c, hipStreamSynchronize(sv));
    HIPCHK(c, hipGetLastError());
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev_va, c->ev_vb) == hipSuccess) c->stats.last_vit_ms = ms / (float)B;
    c->stats.vit_images += (uint64_t)B;
  }
  return DTK_OK;  // IMG (the projected prefix of the cached prefill image) is left untouched
}

// The decoder layers of a prefill: n rows at positions start .. start + n - 1 of a T-token context, X (+ Xn = layer 0's input norm) in,
// X = the last layer's output out, K / V appended at kvbase ([L][2][KVH][Tmax][hd]).  Everything it reads — weights, dimensions, RoPE
// tables, activation and KV scratch — is the context's own: the checkpoint's decoder, or the adapter's embedding model (Adapter::emb).
// pk: the rows are a packed scoring pass instead (dtk_score_packed) — positions, cache rows and the attention's visibility come from its
// tables, T = the cache rows in use; the same kernels by the same rule on n otherwise, so a row's arithmetic is a prefill's.
struct PackedRows { const int2* rope; const int2* seg; int shared_len; };
static void decoder_layers(dtk_ctx* c, int n, int start, int T, bf16_t* kvbase, hipStream_t s, const PackedRows* pk = nullptr) {
  const int hd = c->hd, d = c->d, ff = c->ff;
  const size_t kv_layer = (size_t)2 * c->KVH * c->Tmax * hd;
  auto kc = [&](int l) { return kvbase + (size_t)l * kv_layer; };
  auto vc = [&](int l) { return kvbase + (size_t)l * kv_layer + (size_t)c->KVH * c->Tmax * hd; };
  const float scale = 1.0f / sqrtf((float)hd);
  for (int l = 0; l < c->L; ++l) {
    const LayerW& w = c->layers[l];
    const int qkvn = d + 2 * c->KVH * hd;
    if (!qkv_rope_fused(c, w, n, start, kc(l), vc(l), s, pk ? pk->rope : nullptr)) {
      gemm_role(c, c->Xn, d, w.wqkv, w.p_wqkv, d, nullptr, 0, c->QKV, qkvn, n, qkvn, d, 0, nullptr, nullptr, 0);
      if (pk) launch_rope_scatter_rows(c->QKV, c->Qh, kc(l), vc(l), c->rope_cos, c->rope_sin, n, pk->rope, c->H, c->KVH, c->Tmax, s, hd);
      else launch_rope_scatter(c->QKV, c->Qh, kc(l), vc(l), c->rope_cos, c->rope_sin, n, start, c->H, c->KVH, c->Tmax, s, hd);
    }
    AttnArgs a;
    a.Q = c->Qh; a.q_sh = (long)n * hd; a.q_st = hd;
    a.K = kc(l); a.k_sh = (long)c->Tmax * hd; a.k_st = hd;
    a.V = vc(l); a.v_sh = (long)c->Tmax * hd; a.v_st = hd;
    a.O = c->AO; a.o_sh = hd; a.o_st = d;
    a.H = c->H; a.Tq = n; a.Tk = T; a.hd = hd; a.causal = 1; a.q_offset = start; a.scale = scale; a.impl = c->attn_impl; a.kv_group = c->H / c->KVH;
    if (!pk) launch_attention(a, s);
    else if (!launch_attention_seg(a, pk->shared_len, pk->seg, s)) c->launch_refused = true;
    gemm_role(c, c->AO, d, w.wo, w.p_wo, d, c->X, d, c->X, d, n, d, d, GEMM_RESIDUAL, w.ln2, c->Xn, d);     // + post_attention_layernorm -> Xn
    bool fused = false;      // gate/up + SiLU*mul in one launch where the role is one chain and the shape takes k_gemm_g3 (bit-identical to the pair below)
    if (c->swiglu_fused && w.p_wgui && !c->gemm_naive) {
      GemmArgs g;
      g.A = c->Xn; g.lda = d; g.W = w.wgu; g.Wt = w.p_wgui; g.ldw = d; g.bias = nullptr; g.residual = nullptr; g.ldr = 0;
      g.C = c->ACT; g.ldc = ff; g.M = n; g.N = 2 * ff; g.K = d; g.flags = 0;
      fused = launch_gemm_g3_swiglu(g, s);
    }
    if (!fused && c->swiglu_fused && !c->gemm_naive && c->prefill_sk && n <= SK_CHUNK_ROWS && n <= c->sk_sl_min_rows && (ff % 4) == 0) {
      // a SLICED gate/up role (d = 2048 models): its reduction is SiLU*mul (one chunk of rows; larger prompts take the pair below)
      const int S = std::min(sk_role_slices(2 * ff, d), c->prefill_sk == 1 ? 8 : c->prefill_sk);
      GemmArgs g;
      g.A = c->Xn; g.lda = d; g.W = w.wgu; g.Wt = w.p_wgu; g.ldw = d; g.bias = nullptr; g.residual = nullptr; g.ldr = 0;
      g.C = c->GU; g.ldc = 2 * ff; g.M = n; g.N = 2 * ff; g.K = d; g.flags = 0; g.kslices = S;
      g.part = c->skpart; g.part_stride = (long)SK_CHUNK_ROWS * 2 * ff;
      if (S > 1 && (size_t)S * SK_CHUNK_ROWS * 2 * (size_t)ff <= c->skpart_floats && gemm_sk_supported(g)) {
        if (!launch_gemm_sk_partials(g, s)) c->launch_refused = true;
        else launch_sk_reduce_swiglu(g, c->ACT, ff, s);
        fused = true;
      }
    }
    if (!fused) {
      gemm_role(c, c->Xn, d, w.wgu, w.p_wgu, d, nullptr, 0, c->GU, 2 * ff, n, 2 * ff, d, 0, nullptr, nullptr, 0);
      launch_silu_mul(c->GU, ff, c->ACT, n, s);
    }
    // + the next layer's input_layernorm -> Xn (the final norm runs on the last row only, inside the lm_head GEMV below)
    gemm_role(c, c->ACT, ff, w.wdown, w.p_wdown, ff, c->X, d, c->X, d, n, d, ff, GEMM_RESIDUAL, l + 1 < c->L ? c->layers[l + 1].ln1 : nullptr, c->Xn, d);
  }
}

// The adapter's embedding pass (reference: self.embedding_model(**adapter_inputs).last_hidden_state): T text tokens through the embedding
// model's layers (decoder_layers on its own context) and its final RMSNorm, every row -> c->Xn [T][d].  Synchronous.
static int embed_pass(dtk_ctx* c, const int64_t* ids, int T) {
  if (T < 1 || T > c->Tmax) return fail(c, DTK_ERR_RANGE, "text of %d tokens (the adapter takes 1 .. %d)", T, c->Tmax);
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<int32_t> ids32((size_t)T);
  for (int t = 0; t < T; ++t) {
    if (ids[t] < 0 || ids[t] >= c->V) return fail(c, DTK_ERR_ARG, "text token id %lld out of range", (long long)ids[t]);
    ids32[(size_t)t] = (int32_t)ids[t];
  }
  ensure_prefill_tiles(c);
  hipStream_t s = c->stream;
  HIPCHK(c, hipMemcpyAsync(c->ids_dev, ids32.data(), (size_t)T * 4, hipMemcpyHostToDevice, s));
  launch_embed_gather(c->ids_dev, c->embed, c->X, T, c->d, s);
  c->launch_refused = false;
  launch_rmsnorm_rows(c->X, c->d, c->layers[0].ln1, c->Xn, c->d, T, c->d, c->cfg.rms_eps, s);
  decoder_layers(c, T, 0, T, c->kv, s);
  launch_rmsnorm_rows(c->X, c->d, c->final_norm, c->Xn, c->d, T, c->d, c->cfg.rms_eps, s);
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  if (c->launch_refused) { c->launch_refused = false; return fail(c, DTK_ERR_STATE, "embedding pass: a sliced-K projection was refused by its kernel"); }
  return DTK_OK;
}

// Connector output and every cross layer's k / v for this text, unless they are cached already (same ids).  Synchronous, on stream s.
static int text_prepare(dtk_ctx* c, const int64_t* ids, int T, hipStream_t s) {
  Adapter& A = *c->ad;
  if (!ids || T < 1 || T > A.cfg.text_max) return fail(c, DTK_ERR_RANGE, "text of %d tokens (the adapter takes 1 .. %d)", T, A.cfg.text_max);
  if ((int)A.text_ids.size() == T && std::equal(ids, ids + T, A.text_ids.begin())) return DTK_OK;
  A.text_ids.clear();
  dtk_ctx* e = A.emb;
  if (embed_pass(e, ids, T) != DTK_OK) return fail(c, DTK_ERR_STATE, "adapter embedding pass: %s", e->err.c_str());
  struct StreamScope { dtk_ctx* c; hipStream_t prev; ~StreamScope() { c->cur_stream = prev; } } scope{c, c->cur_stream};
  c->cur_stream = s;
  const int D = c->vD, hd = c->vHd, de = e->d;
  gemm(c, e->Xn, de, A.conn_w, de, A.conn_b, nullptr, 0, A.ctext, D, T, D, de, GEMM_BIAS);
  for (size_t i = 0; i < A.layers.size(); ++i) {
    if (!A.present[i]) continue;
    const CrossW& w = A.layers[i];
    gemm(c, A.ctext, D, w.kw, D, w.kb, nullptr, 0, w.K, D, T, D, D, GEMM_BIAS);
    launch_layernorm_rows(w.K, hd, w.knw, w.knb, w.K, hd, T * c->vH, hd, c->cfg.vit_ln_eps, s);   // k_norm per head, in place
    gemm(c, A.ctext, D, w.vw, D, w.vb, nullptr, 0, w.V, D, T, D, D, GEMM_BIAS);
  }
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  A.text_ids.assign(ids, ids + T);
  return DTK_OK;
}

// dummy_input.clamp(-1, 1) as fp32 pixels, `batch` times (the text-only prompt's image, reference add_hooks.forward_hook)
static int dummy_pixels(dtk_ctx* c, int batch, std::vector<float>& out) {
  Adapter& A = *c->ad;
  const size_t img = (size_t)3 * c->cfg.vit_image * c->cfg.vit_image;
  if (A.dummy_host.empty()) {
    std::vector<uint16_t> bits(img);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(bits.data(), A.dummy, img * 2, hipMemcpyDeviceToHost));
    A.dummy_host.resize(img);
    for (size_t k = 0; k < img; ++k) A.dummy_host[k] = std::min(1.f, std::max(-1.f, host_bf2f(bits[k])));
  }
  out.resize(img * (size_t)batch);
  for (int b = 0; b < batch; ++b) std::copy(A.dummy_host.begin(), A.dummy_host.end(), out.begin() + (size_t)b * img);
  return DTK_OK;
}

// dtk_score's rider on a prefill: the log-probabilities of ids[first .. T-1] from the hidden states of rows first-1 .. T-2
// k > 0 (dtk_score_top): + every scored position's k most likely tokens, [rows][k] ids and log-probabilities
struct ScoreReq { int first; float* logprob; int32_t* argmax; float* lse; int k = 0; int32_t* top_ids = nullptr; float* top_logprob = nullptr; };

static int score_buffers(dtk_ctx* c, int k = 0) {
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->score_rec) HIPCHK(c, hipMalloc(&c->score_rec, score_rec_floats(c->Tmax, c->V) * sizeof(float)));
  if (!c->score_out) HIPCHK(c, hipMalloc(&c->score_out, (size_t)4 * c->Tmax * sizeof(float)));
  if (k > 0 && !c->score_top) HIPCHK(c, hipMalloc(&c->score_top, (size_t)2 * c->Tmax * DTK_MAX_TOP * sizeof(float)));
  return DTK_OK;
}
// the k / top_ids_out / top_logprob_out triple of the *_top calls: k = 0 with both NULL is the call without them
static int top_check(dtk_ctx* c, const char* who, int k, const int32_t* top_ids_out, const float* top_logprob_out) {
  if (k == 0 && !top_ids_out && !top_logprob_out) return DTK_OK;
  if (k < 1 || k > DTK_MAX_TOP) return fail(c, DTK_ERR_ARG, "%s: k = %d (1 .. DTK_MAX_TOP = %d, or 0 with NULL outputs)", who, k, DTK_MAX_TOP);
  if (k > c->V) return fail(c, DTK_ERR_ARG, "%s: k = %d exceeds the vocabulary (%d)", who, k, c->V);
  if (!top_ids_out || !top_logprob_out) return fail(c, DTK_ERR_ARG, "%s: k = %d needs top_ids_out and top_logprob_out", who, k);
  return DTK_OK;
}
// the device -> host copies of a scoring call's top-k results (rows x k, contiguous)
static int score_top_copy(dtk_ctx* c, int M, int k, int32_t* top_ids, float* top_logprob, hipStream_t s) {
  if (k <= 0) return DTK_OK;
  HIPCHK(c, hipMemcpyAsync(top_ids, c->score_top, (size_t)M * k * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(top_logprob, c->score_top + (size_t)c->Tmax * DTK_MAX_TOP, (size_t)M * k * 4, hipMemcpyDeviceToHost, s));
  return DTK_OK;
}

// final norm of M rows of X -> Xn, lm_head with the log-softmax epilogue, merge: results in c->score_out.  targets: device, one per row
static int score_rows(dtk_ctx* c, const bf16_t* X, int M, const int32_t* targets, hipStream_t s, int k = 0) {
  const int d = c->d;
  launch_rmsnorm_rows(X, d, c->final_norm, c->Xn, d, M, d, c->cfg.rms_eps, s);
  GemmArgs g;
  g.A = c->Xn; g.lda = d; g.W = c->lm_head; g.ldw = d; g.bias = nullptr; g.residual = nullptr; g.ldr = 0; g.C = nullptr; g.ldc = 0;
  g.Wt = (c->t_lm_head && c->tiled_ready) ? c->t_lm_head : nullptr;
  g.M = M; g.N = c->V; g.K = d; g.flags = 0; g.ls_target = targets; g.ls_rec = c->score_rec;
  if (!launch_gemm_logsoftmax(g, s)) return fail(c, DTK_ERR_STATE, "dtk_score: the log-softmax lm_head kernel does not take this shape (d = %d)", d);
  float* o = c->score_out;
  launch_score_merge(c->score_rec, M, c->V, o, o + c->Tmax, reinterpret_cast<int32_t*>(o + 2 * (size_t)c->Tmax), o + 3 * (size_t)c->Tmax, s);
  if (k > 0)
    launch_score_top(g, o + c->Tmax, k, reinterpret_cast<int32_t*>(c->score_top), c->score_top + (size_t)c->Tmax * DTK_MAX_TOP, nullptr, s);
  return DTK_OK;
}

static int prefill_impl(dtk_ctx* c, SeqHost& sh, bf16_t* kvbase, float* logits_dst, DecState* st_dst, bool is_single,
                        const int64_t* ids, int T, const float* pixels, uint64_t image_key, int flags, float* logits_out,
                        const int64_t* text_ids = nullptr, int T_text = 0, const ScoreReq* score = nullptr) {
  if (!c || !ids || T < 1) return fail(c, DTK_ERR_ARG, "dtk_prefill: bad argument");
  if (T > c->Tmax) return fail(c, DTK_ERR_RANGE, "prompt of %d tokens exceeds max_positions %d", T, c->Tmax);
  if (!is_single && c->spec_on) return fail(c, DTK_ERR_STATE, "prefill into a slot while slot 0 is speculating (dtk_spec_end first)");
  std::lock_guard<std::mutex> vit_guard(c->vit_mu);
  HIPCHK(c, hipSetDevice(c->device));
  // drain pending decode steps (their tokens are dropped)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  ensure_prefill_tiles(c);
  if (is_single) c->waited = c->launched = 0;  // the device draw counter restarts with this prefill
  else c->bwaited = c->blaunched;
  // ---- locate the image placeholder run (reference v1/modeling_detikzify.py:179-184)
  int img_start = -1, img_count = 0;
  for (int t = 0; t < T; ++t) {
    if (ids[t] < 0 || ids[t] >= c->V) return fail(c, DTK_ERR_ARG, "token id %lld out of range", (long long)ids[t]);
    if (ids[t] == c->cfg.image_token_id) { if (img_start < 0) img_start = t; img_count++; }
  }
  const bool has_img = img_count > 0;
  const bool use_img = has_img && (pixels != nullptr || ((flags & DTK_PREFILL_REUSE_IMAGE) && c->have_image && c->cached_image_key == image_key));
  if (use_img) {
    if (img_count != c->nImg)
      return fail(c, DTK_ERR_ARG, "The number of image patch tokens should be the same as the number of image patches.");
    for (int t = 0; t < c->nImg; ++t)
      if (ids[img_start + t] != c->cfg.image_token_id)
        return fail(c, DTK_ERR_ARG, "The image patch tokens should be consecutive.");
  }
  HIPCHK(c, hipEventRecord(c->ev_a, c->stream));
  // ---- longest common prefix with the cached sequence (output-identical KV reuse).  The KV of the image positions
  // depends on the image, not on the (all equal) placeholder ids: the cached sequence must have been computed with the
  // same image key, and with / without spliced image features never mixes.
  int start = 0;
  const bool same_image = !has_img || (sh.cached_with_image == use_img && (!use_img || (image_key != 0 && sh.image_key == image_key)));
  if ((flags & DTK_PREFILL_REUSE_PREFIX) && same_image && !sh.cached_ids.empty()) {
    int lim = (int)std::min<size_t>(sh.cached_ids.size(), (size_t)T - 1);
    if (score) lim = std::min(lim, score->first - 1);      // the scored rows' hidden states are computed here, whatever the cache holds
    while (start < lim && sh.cached_ids[start] == ids[start]) ++start;
  }
  // ---- image features are needed only if an image position has to be recomputed
  if (use_img && start < img_start + c->nImg) {
    const bool reuse = (flags & DTK_PREFILL_REUSE_IMAGE) && c->have_image && c->cached_image_key == image_key;
    if (!reuse) {
      if (!pixels) return fail(c, DTK_ERR_ARG, "pixels required (no cached image for this key)");
      const size_t img = (size_t)3 * c->cfg.vit_image * c->cfg.vit_image;
      HIPCHK(c, hipMemcpyAsync(c->pixels_dev, pixels, img * 4, hipMemcpyHostToDevice, c->stream));
      if (text_ids) { const int rc = text_prepare(c, text_ids, T_text, c->stream); if (rc != DTK_OK) return rc; }
      vit_forward(c, false, c->stream, 1, text_ids != nullptr);
      project_image(c);
      c->stats.vit_images++;
      c->have_image = true;
      c->cached_image_key = image_key;
    }
  }
  HIPCHK(c, hipEventRecord(c->ev_b, c->stream));
  sh.last_reuse_start = start;
  const int n = T - start;
  std::vector<int32_t> ids32((size_t)n);
  for (int t = 0; t < n; ++t) ids32[(size_t)t] = (int32_t)ids[start + t];
  HIPCHK(c, hipMemcpyAsync(c->ids_dev, ids32.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  hipStream_t s = c->stream;
  const int d = c->d;
  launch_embed_gather(c->ids_dev, c->embed, c->X, n, d, s);
  if (use_img) {  // splice projected image features over the placeholder embeddings
    const int lo = std::max(img_start, start), hi = img_start + c->nImg;
    if (hi > lo) launch_copy_rows(c->IMG + (size_t)(lo - img_start) * d, d, c->X + (size_t)(lo - start) * d, d, hi - lo, d, s);
  }
  c->launch_refused = false;      // (a batched step that was refused leaves it set: this prefill judges its own launches)
  launch_rmsnorm_rows(c->X, d, c->layers[0].ln1, c->Xn, d, n, d, c->cfg.rms_eps, s);
  decoder_layers(c, n, start, T, kvbase, s);
  if (c->launch_refused) { c->launch_refused = false; return fail(c, DTK_ERR_STATE, "prefill: a sliced-K projection was refused by its kernel (nothing launched for it)"); }
  // final norm + lm_head on the last position only (the sampler consumes logits[:, -1])
  GemvArgs g{};
  g.W = c->lm_head; g.W8 = c->q_lm_head; g.wscale = c->s_lm_head; g.N = c->V; g.K = d; g.x = c->X + (size_t)(n - 1) * d; g.norm_w = c->final_norm;
  g.eps = c->cfg.rms_eps; g.logits = logits_dst;
  launch_gemv(PRO_RMSNORM, EPI_LOGITS, g, s);
  DecState st0{};
  st0.pos = T - 1; st0.next_pos = T; st0.token = (int32_t)ids[T - 1]; st0.draw = 0;
  HIPCHK(c, hipMemcpyAsync(st_dst, &st0, sizeof st0, hipMemcpyHostToDevice, s));
  if (score) {
    // rows first-1 .. T-2 of the context = rows first-1-start .. of X; the target of row p is ids[p + 1], already on the device
    const int rc = score_rows(c, c->X + (size_t)(score->first - 1 - start) * d, T - score->first, c->ids_dev + (score->first - start), s, score->k);
    if (rc != DTK_OK) return rc;
  }
  HIPCHK(c, hipEventRecord(c->ev_c, s));      // stats.last_prefill_ms of a scoring call includes its lm_head pass
  if (logits_out) HIPCHK(c, hipMemcpyAsync(logits_out, logits_dst, (size_t)c->V * 4, hipMemcpyDeviceToHost, s));
  if (score) {
    const int M = T - score->first;
    const float* o = c->score_out;
    HIPCHK(c, hipMemcpyAsync(score->logprob, o, (size_t)M * 4, hipMemcpyDeviceToHost, s));
    if (score->lse) HIPCHK(c, hipMemcpyAsync(score->lse, o + c->Tmax, (size_t)M * 4, hipMemcpyDeviceToHost, s));
    if (score->argmax) HIPCHK(c, hipMemcpyAsync(score->argmax, o + 2 * (size_t)c->Tmax, (size_t)M * 4, hipMemcpyDeviceToHost, s));
    const int rc = score_top_copy(c, M, score->k, score->top_ids, score->top_logprob, s);
    if (rc != DTK_OK) return rc;
  }
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, c->ev_a, c->ev_c) == hipSuccess) c->stats.last_prefill_ms = ms;
  if (hipEventElapsedTime(&ms, c->ev_a, c->ev_b) == hipSuccess) c->stats.last_vit_ms = ms;
  c->stats.prefill_tokens += (uint64_t)n;
  sh.cached_ids.assign(ids, ids + T);
  sh.forced_pending = -1;
  if (const int rc = pen_rebuild(c, pen_index(c, sh), ids, T)) return rc;
  sh.cached_with_image = use_img;
  sh.image_key = use_img ? image_key : 0;
  sh.host_next_pos = T;
  sh.have_logits = true;
  // a new prefill starts a new generation: reset the draw counter of the sampler
  return DTK_OK;
}

int dtk_prefill(dtk_ctx* c, const int64_t* ids, int T, const float* pixels, uint64_t image_key, int flags, float* logits_out) {
  if (!c) return DTK_ERR_ARG;
  return prefill_impl(c, c->seq0, c->kv, c->logits, c->st, true, ids, T, pixels, image_key, flags, logits_out);
}

// argument checks of dtk_score / dtk_score_text: everything is refused before anything is launched
static int score_check(dtk_ctx* c, const int64_t* ids, int T, int first, const float* logprob_out, int k = 0, const int32_t* top_ids_out = nullptr,
                       const float* top_logprob_out = nullptr) {
  if (!ids || !logprob_out) return fail(c, DTK_ERR_ARG, "dtk_score: null argument");
  if (T < 2) return fail(c, DTK_ERR_ARG, "dtk_score: %d token(s): scoring needs a context token and a target (T >= 2)", T);
  if (T > c->Tmax) return fail(c, DTK_ERR_RANGE, "dtk_score: %d tokens exceed max_positions %d", T, c->Tmax);
  if (first < 1 || first > T - 1) return fail(c, DTK_ERR_ARG, "dtk_score: first = %d (the first scored target position: 1 .. T-1 = %d)", first, T - 1);
  for (int t = first; t < T; ++t)
    if (ids[t] < 0 || ids[t] >= c->V) return fail(c, DTK_ERR_ARG, "dtk_score: target id %lld at position %d outside [0, %d)", (long long)ids[t], t, c->V);
  if (!gemm_logsoftmax_supported(c->d)) return fail(c, DTK_ERR_ARG, "dtk_score: the log-softmax lm_head kernel needs hidden %% 8 == 0 (d = %d)", c->d);
  const int rc = top_check(c, "dtk_score_top", k, top_ids_out, top_logprob_out);
  if (rc != DTK_OK) return rc;
  return score_buffers(c, k);
}

int dtk_score_top(dtk_ctx* c, const int64_t* ids, int T, const float* pixels, uint64_t image_key, uint32_t flags, int first,
                  float* logprob_out, int32_t* argmax_out, float* lse_out, int k, int32_t* top_ids_out, float* top_logprob_out) {
  if (!c) return DTK_ERR_ARG;
  const int rc = score_check(c, ids, T, first, logprob_out, k, top_ids_out, top_logprob_out);
  if (rc != DTK_OK) return rc;
  const ScoreReq rq{first, logprob_out, argmax_out, lse_out, k, top_ids_out, top_logprob_out};
  return prefill_impl(c, c->seq0, c->kv, c->logits, c->st, true, ids, T, pixels, image_key, (int)flags, nullptr, nullptr, 0, &rq);
}

int dtk_score(dtk_ctx* c, const int64_t* ids, int T, const float* pixels, uint64_t image_key, uint32_t flags, int first,
              float* logprob_out, int32_t* argmax_out, float* lse_out) {
  return dtk_score_top(c, ids, T, pixels, image_key, flags, first, logprob_out, argmax_out, lse_out, 0, nullptr, nullptr);
}

// ---- dtk_score_packed: N candidate continuations of one prompt in ONE pass of the decoder layers -------------------
// Rows: the prompt's positions start .. P-2 (ordinary causal rows, K / V at cache row = position), then one segment per candidate with
// the input tokens prefix[P-1], cand_i[0 .. len_i-2] at positions P-1 + j and cache rows P-1 + b_i + j (b_i = the lengths before it).
struct PackedReq {
  const int64_t* prefix; int P;
  const int64_t* cand_ids; const int32_t* cand_len; int N;
  float* logprob; int32_t* argmax; float* lse;
  int k = 0; int32_t* top_ids = nullptr; float* top_logprob = nullptr;      // dtk_score_packed_top
};

// every refusal of dtk_score_packed / dtk_score_packed_text, before anything is launched or the context changes; total = sum of len_i
static int packed_check(dtk_ctx* c, const PackedReq& r, int* total_out) {
  if (!r.prefix || !r.cand_ids || !r.cand_len || !r.logprob) return fail(c, DTK_ERR_ARG, "dtk_score_packed: null argument");
  if (r.P < 1) return fail(c, DTK_ERR_ARG, "dtk_score_packed: a prompt of %d tokens (P >= 1)", r.P);
  if (r.N < 1) return fail(c, DTK_ERR_ARG, "dtk_score_packed: %d candidates (N >= 1)", r.N);
  long total = 0;
  for (int i = 0; i < r.N; ++i) {
    if (r.cand_len[i] < 1) return fail(c, DTK_ERR_ARG, "dtk_score_packed: candidate %d has %d tokens (len >= 1)", i, r.cand_len[i]);
    total += r.cand_len[i];
  }
  if ((long)r.P - 1 + total > (long)c->Tmax)
    return fail(c, DTK_ERR_RANGE, "dtk_score_packed: %d prompt + %ld candidate rows exceed max_positions %d", r.P - 1, total, c->Tmax);
  for (int t = 0; t < r.P; ++t)
    if (r.prefix[t] < 0 || r.prefix[t] >= c->V) return fail(c, DTK_ERR_ARG, "dtk_score_packed: token id %lld out of range", (long long)r.prefix[t]);
  for (long k = 0; k < total; ++k) {
    if (r.cand_ids[k] < 0 || r.cand_ids[k] >= c->V)
      return fail(c, DTK_ERR_ARG, "dtk_score_packed: candidate id %lld at %ld outside [0, %d)", (long long)r.cand_ids[k], k, c->V);
  }
  if (c->attn_impl == 1)
    return fail(c, DTK_ERR_STATE, "dtk_score_packed: attn_impl = 1 (the VALU attention kernel) has no segmented form; the packed pass needs the MFMA kernel (attn_impl 0 or 2)");
  if (!gemm_logsoftmax_supported(c->d)) return fail(c, DTK_ERR_ARG, "dtk_score_packed: the log-softmax lm_head kernel needs hidden %% 8 == 0 (d = %d)", c->d);
  const int rct = top_check(c, "dtk_score_packed_top", r.k, r.top_ids, r.top_logprob);
  if (rct != DTK_OK) return rct;
  const int rc = score_buffers(c, r.k);
  if (rc != DTK_OK) return rc;
  if (!c->packed_rows) HIPCHK(c, hipMalloc(&c->packed_rows, (size_t)6 * c->Tmax * sizeof(int32_t)));
  *total_out = (int)total;
  return DTK_OK;
}

static int score_packed_impl(dtk_ctx* c, const PackedReq& r, int total, const float* pixels, uint64_t image_key, int flags,
                             const int64_t* text_ids = nullptr, int T_text = 0) {
  SeqHost& sh = c->seq0;
  const int P = r.P, shared = P - 1;
  // ---- the image placeholder run of the prompt, as prefill_impl locates and checks it
  int img_start = -1, img_count = 0;
  for (int t = 0; t < P; ++t)
    if (r.prefix[t] == c->cfg.image_token_id) { if (img_start < 0) img_start = t; img_count++; }
  const bool has_img = img_count > 0;
  const bool image_given = pixels != nullptr || ((flags & DTK_PREFILL_REUSE_IMAGE) && c->have_image && c->cached_image_key == image_key);
  const bool use_img = has_img && image_given;
  if (use_img) {
    if (img_count != c->nImg)
      return fail(c, DTK_ERR_ARG, "The number of image patch tokens should be the same as the number of image patches.");
    for (int t = 0; t < c->nImg; ++t)
      if (r.prefix[img_start + t] != c->cfg.image_token_id)
        return fail(c, DTK_ERR_ARG, "The image patch tokens should be consecutive.");
  }
  // a placeholder inside a candidate: without an image it is a token like any other, as in dtk_score; with one, dtk_score(prefix +
  // cand_i) would count it among the image's (one more than the image has, or a run that leaves the prompt): the image run must lie
  // in the prompt
  if (image_given)
    for (int k = 0; k < total; ++k)
      if (r.cand_ids[k] == c->cfg.image_token_id)
        return fail(c, DTK_ERR_ARG, "The number of image patch tokens should be the same as the number of image patches.");
  // ---- longest common prefix with the cached sequence, capped at P-1: position P-1 is computed once per candidate
  int start = 0;
  const bool same_image = !has_img || (sh.cached_with_image == use_img && (!use_img || (image_key != 0 && sh.image_key == image_key)));
  if ((flags & DTK_PREFILL_REUSE_PREFIX) && same_image && !sh.cached_ids.empty()) {
    const int lim = (int)std::min<size_t>(sh.cached_ids.size(), (size_t)shared);
    while (start < lim && sh.cached_ids[start] == r.prefix[start]) ++start;
  }
  const bool need_img = use_img && start < img_start + c->nImg;
  const bool reuse_img = (flags & DTK_PREFILL_REUSE_IMAGE) && c->have_image && c->cached_image_key == image_key;
  if (need_img && !reuse_img && !pixels) return fail(c, DTK_ERR_ARG, "pixels required (no cached image for this key)");
  // ---- nothing is refused from here on
  std::lock_guard<std::mutex> vit_guard(c->vit_mu);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));     // drain pending decode steps (their tokens are dropped)
  ensure_prefill_tiles(c);
  c->waited = c->launched = 0;
  // the cache rows from `start` on are rewritten: whatever happens below, the context holds no sequence to decode from
  sh.cached_ids.resize((size_t)start);
  sh.forced_pending = -1;
  if (const int rc = pen_rebuild(c, pen_index(c, sh), nullptr, 0)) return rc;     // no sequence from here on, whatever happens below: an empty table
  sh.have_logits = false;
  sh.host_next_pos = start;
  hipStream_t s = c->stream;
  HIPCHK(c, hipEventRecord(c->ev_a, s));
  if (need_img && !reuse_img) {
    const size_t img = (size_t)3 * c->cfg.vit_image * c->cfg.vit_image;
    HIPCHK(c, hipMemcpyAsync(c->pixels_dev, pixels, img * 4, hipMemcpyHostToDevice, s));
    if (text_ids) { const int rc = text_prepare(c, text_ids, T_text, s); if (rc != DTK_OK) return rc; }
    vit_forward(c, false, s, 1, text_ids != nullptr);
    project_image(c);
    c->stats.vit_images++;
    c->have_image = true;
    c->cached_image_key = image_key;
  }
  HIPCHK(c, hipEventRecord(c->ev_b, s));
  sh.last_reuse_start = start;
  // ---- the row tables
  const int n_shared = shared - start, n = n_shared + total, Tm = c->Tmax;
  std::vector<int32_t> tab((size_t)6 * Tm);
  int32_t *rope = tab.data(), *seg = rope + 2 * (size_t)Tm, *ids32 = seg + 2 * (size_t)Tm, *targets = ids32 + Tm;
  for (int t = 0; t < n_shared; ++t) {
    rope[2 * t] = start + t; rope[2 * t + 1] = start + t;
    seg[2 * t] = 0; seg[2 * t + 1] = start + t;
    ids32[t] = (int32_t)r.prefix[start + t];
  }
  {
    int row = n_shared, k = 0;
    for (int i = 0; i < r.N; ++i) {
      const int begin = shared + k;     // cache row of the segment's first row: k = b_i
      for (int j = 0; j < r.cand_len[i]; ++j, ++row, ++k) {
        rope[2 * row] = shared + j; rope[2 * row + 1] = begin + j;
        seg[2 * row] = begin; seg[2 * row + 1] = begin + j;
        ids32[row] = (int32_t)(j == 0 ? r.prefix[P - 1] : r.cand_ids[k - 1]);
        targets[k] = (int32_t)r.cand_ids[k];
      }
    }
  }
  int32_t* dtab = c->packed_rows;
  const int2* d_rope = reinterpret_cast<const int2*>(dtab);
  const int2* d_seg = reinterpret_cast<const int2*>(dtab + 2 * (size_t)Tm);
  const int32_t *d_ids = dtab + 4 * (size_t)Tm, *d_targets = dtab + 5 * (size_t)Tm;
  // only the used part of each table travels; `tab` is pageable host memory, so the error returns below drain the stream first
  HIPCHK(c, hipMemcpyAsync(dtab, rope, (size_t)2 * n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(dtab + 2 * (size_t)Tm, seg, (size_t)2 * n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(dtab + 4 * (size_t)Tm, ids32, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(dtab + 5 * (size_t)Tm, targets, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice, s));
  const int d = c->d;
  launch_embed_gather(d_ids, c->embed, c->X, n, d, s);
  if (use_img) {  // splice projected image features over the placeholder embeddings: the prompt's rows, and position P-1's copies
    const int lo = std::max(img_start, start), hi = std::min(img_start + c->nImg, shared);
    if (hi > lo) launch_copy_rows(c->IMG + (size_t)(lo - img_start) * d, d, c->X + (size_t)(lo - start) * d, d, hi - lo, d, s);
    if (shared >= img_start && shared < img_start + c->nImg) {
      int row = n_shared;
      for (int i = 0; i < r.N; row += r.cand_len[i], ++i)
        launch_copy_rows(c->IMG + (size_t)(shared - img_start) * d, d, c->X + (size_t)row * d, d, 1, d, s);
    }
  }
  c->launch_refused = false;
  launch_rmsnorm_rows(c->X, d, c->layers[0].ln1, c->Xn, d, n, d, c->cfg.rms_eps, s);
  const PackedRows pk{d_rope, d_seg, shared};
  decoder_layers(c, n, start, shared + total, c->kv, s, &pk);
  if (c->launch_refused) {
    c->launch_refused = false;
    (void)hipStreamSynchronize(s);
    return fail(c, DTK_ERR_STATE, "dtk_score_packed: a kernel refused its shape (nothing launched for it)");
  }
  const int rc = score_rows(c, c->X + (size_t)n_shared * d, total, d_targets, s, r.k);
  if (rc != DTK_OK) { (void)hipStreamSynchronize(s); return rc; }
  HIPCHK(c, hipEventRecord(c->ev_c, s));
  const float* o = c->score_out;
  HIPCHK(c, hipMemcpyAsync(r.logprob, o, (size_t)total * 4, hipMemcpyDeviceToHost, s));
  if (r.lse) HIPCHK(c, hipMemcpyAsync(r.lse, o + Tm, (size_t)total * 4, hipMemcpyDeviceToHost, s));
  if (r.argmax) HIPCHK(c, hipMemcpyAsync(r.argmax, o + 2 * (size_t)Tm, (size_t)total * 4, hipMemcpyDeviceToHost, s));
  { const int rct = score_top_copy(c, total, r.k, r.top_ids, r.top_logprob, s); if (rct != DTK_OK) { (void)hipStreamSynchronize(s); return rct; } }
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, c->ev_a, c->ev_c) == hipSuccess) c->stats.last_prefill_ms = ms;
  if (hipEventElapsedTime(&ms, c->ev_a, c->ev_b) == hipSuccess) c->stats.last_vit_ms = ms;
  c->stats.prefill_tokens += (uint64_t)n;
  // the prompt's first P-1 positions stay; no current sequence (have_logits is false: dtk_decode refuses until the next prefill)
  sh.cached_ids.assign(r.prefix, r.prefix + shared);
  sh.cached_with_image = use_img;
  sh.image_key = use_img ? image_key : 0;
  sh.host_next_pos = shared;
  return DTK_OK;
}

int dtk_score_packed_top(dtk_ctx* c, const int64_t* prefix_ids, int P, const float* pixels, uint64_t image_key, uint32_t flags,
                         const int64_t* cand_ids, const int32_t* cand_len, int N, float* logprob_out, int32_t* argmax_out, float* lse_out,
                         int k, int32_t* top_ids_out, float* top_logprob_out) {
  if (!c) return DTK_ERR_ARG;
  const PackedReq rq{prefix_ids, P, cand_ids, cand_len, N, logprob_out, argmax_out, lse_out, k, top_ids_out, top_logprob_out};
  int total = 0;
  const int rc = packed_check(c, rq, &total);
  if (rc != DTK_OK) return rc;
  return score_packed_impl(c, rq, total, pixels, image_key, (int)flags);
}

int dtk_score_packed(dtk_ctx* c, const int64_t* prefix_ids, int P, const float* pixels, uint64_t image_key, uint32_t flags,
                     const int64_t* cand_ids, const int32_t* cand_len, int N, float* logprob_out, int32_t* argmax_out, float* lse_out) {
  return dtk_score_packed_top(c, prefix_ids, P, pixels, image_key, flags, cand_ids, cand_len, N, logprob_out, argmax_out, lse_out, 0, nullptr, nullptr);
}

int dtk_prefill_slot(dtk_ctx* c, int slot, const int64_t* ids, int T, const float* pixels, uint64_t image_key, int flags, float* logits_out) {
  if (!c || slot < 0 || slot >= c->nb) return fail(c, DTK_ERR_ARG, "dtk_prefill_slot: slot %d of %d", slot, c ? c->nb : 0);
  SeqHost& sh = c->bseq[(size_t)slot];
  sh.last_reuse_start = 0;
  const int rc = prefill_impl(c, sh, c->kvb + (size_t)slot * c->kv_slot_stride, c->logits_b + (size_t)slot * c->V,
                              c->st_b + slot, false, ids, T, pixels, image_key, flags, logits_out);
  // positions >= kept of this slot were (or may have been) rewritten: shared-prefix reads stay valid only below that
  const int kept = rc == DTK_OK ? sh.last_reuse_start : 0;
  auto clip = [&](SeqHost& q) { q.share_len = std::min(q.share_len, kept); if (q.share_len <= 0) { q.share_src = -1; q.share_len = 0; } };
  clip(sh);
  for (int j = 0; j < c->nb; ++j)
    if (j != slot && c->bseq[(size_t)j].share_src == slot) clip(c->bseq[(size_t)j]);
  if (rc == DTK_OK) sh.kv8_from = sh.host_next_pos;      // every row of the slot is now a prefill row (kept ones included): bf16 only
  else sh.kv8_from = std::min(sh.kv8_from, sh.host_next_pos);      // a refused or failed prefill may have cut the context: never above its length
  return rc;
}

static int set_sampling_impl(dtk_ctx* c, const dtk_sampling* sp, SamplingDev* sp_dst, DecState* st_dst, bool is_single) {
  if (!c || !sp) return fail(c, DTK_ERR_ARG, "dtk_set_sampling: null argument");
  if (sp->n_bad < 0 || sp->n_bad > 8 || sp->n_begin_suppress < 0 || sp->n_begin_suppress > 8 ||
      sp->n_always_suppress < 0 || sp->n_always_suppress > 8)
    return fail(c, DTK_ERR_ARG, "at most 8 ids per suppression list");
  if (sp->do_sample && !(sp->temperature > 0.f)) return fail(c, DTK_ERR_ARG, "temperature must be > 0");
  if (sp->do_sample && !(sp->top_p > 0.f && sp->top_p <= 1.f)) return fail(c, DTK_ERR_ARG, "top_p must be in (0, 1]");
  HIPCHK(c, hipSetDevice(c->device));
  SamplingDev dv{};
  dv.do_sample = sp->do_sample; dv.temperature = sp->temperature; dv.top_p = sp->top_p; dv.top_k = sp->top_k;
  dv.seed = sp->seed;
  dv.n_bad = sp->n_bad; dv.n_begin = sp->n_begin_suppress; dv.n_always = sp->n_always_suppress;
  for (int i = 0; i < 8; ++i) {
    dv.bad_ids[i] = sp->bad_ids[i]; dv.begin_ids[i] = sp->begin_suppress_ids[i]; dv.always_ids[i] = sp->always_suppress_ids[i];
  }
  if (!is_single && c->sp_stage) {
    // a slot's parameters change between two of ITS sequences, while a step of the OTHER slots may be in flight: the upload is
    // queued behind that step from a pinned per-slot staging record (rewritten only at the slot's next set_sampling, sequences
    // later) instead of draining the stream — a drain per join cost the batch a ~5 ms bubble (128 joins: 0.57 s of a 8 s search)
    const int slot = (int)(sp_dst - c->sp_b);
    c->sp_stage[slot] = dv;
    c->draw_stage[slot] = 0;
    HIPCHK(c, hipMemcpyAsync(sp_dst, &c->sp_stage[slot], sizeof dv, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(&st_dst->draw, &c->draw_stage[slot], sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  } else {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(sp_dst, &dv, sizeof dv, hipMemcpyHostToDevice));
    const uint32_t zero = 0;
    HIPCHK(c, hipMemcpy(&st_dst->draw, &zero, sizeof zero, hipMemcpyHostToDevice));
  }
  if (is_single) { c->sampling = *sp; c->launched = c->waited = 0; c->sampling_ext = dtk_sampling_ext{}; c->trunc_single = false; }
  else c->slot_trunc[(int)(sp_dst - c->sp_b)] = false;      // dv.qmin = dv.eps = 0: dtk_set_sampling_*_ext follows where they are wanted
  if (const int rc = pen_set(c, is_single ? 0 : 1 + (int)(sp_dst - c->sp_b), 0.f, 0.f, 0)) return rc;      // dtk_set_penalties[_slot] likewise
  if (const int rc = dry_set(c, is_single ? 0 : 1 + (int)(sp_dst - c->sp_b), nullptr)) return rc;      // dtk_set_dry[_slot] likewise
  if (const int rc = len_set(c, is_single ? 0 : 1 + (int)(sp_dst - c->sp_b), nullptr)) return rc;      // dtk_set_length_control[_slot] and
  if (const int rc = bias_set(c, is_single ? 0 : 1 + (int)(sp_dst - c->sp_b), nullptr, nullptr, 0)) return rc;      // dtk_set_logit_bias[_slot] likewise
  // which sampler the captured graphs must contain: the multi-block chain serves large vocabularies unless a
  // configuration needs top-k; a change of kind drops the graph (re-captured by the next launch)
  const bool needs_topk = sp->do_sample && sp->top_k > 0 && sp->top_k < c->V;
  if (is_single) {
    const bool mb = sample_mb_preferred(c->V, sp->do_sample != 0) && !needs_topk;
    if (mb != c->mb_single) {
      c->mb_single = mb;
      if (c->graph_exec) { (void)hipGraphExecDestroy(c->graph_exec); c->graph_exec = nullptr; }
      if (c->graph) { (void)hipGraphDestroy(c->graph); c->graph = nullptr; }
      if (c->graph_short_exec) { (void)hipGraphExecDestroy(c->graph_short_exec); c->graph_short_exec = nullptr; }
      if (c->graph_short) { (void)hipGraphDestroy(c->graph_short); c->graph_short = nullptr; }
      c->graph_ready = false;
    }
  } else {
    const int slot = (int)(sp_dst - c->sp_b);
    c->slot_topk[slot] = needs_topk;
    c->slot_samples[slot] = sp->do_sample != 0;
    bool any = false, any_sampling = false;
    for (int j = 0; j < c->nb; ++j) { any = any || c->slot_topk[j]; any_sampling = any_sampling || c->slot_samples[j]; }
    const bool mb = sample_mb_preferred(c->V, any_sampling) && !any;
    if (mb != c->mb_batch) {
      c->mb_batch = mb;
      drop_batch_graphs(c);
    }
    bool tr = false;
    for (int j = 0; j < c->nb; ++j) tr = tr || c->slot_trunc[j];
    c->trunc_batch = tr;
  }
  return DTK_OK;
}

// min_p / epsilon_cutoff of the configuration the last dtk_set_sampling[_slot] left at sp_dst: the two fields alone are rewritten
extern "C++" int ext_check(dtk_ctx* c, const dtk_sampling_ext* x, const char* who) {
  if (!x) return fail(c, DTK_ERR_ARG, "%s: null argument", who);
  if (!(x->min_p >= 0.f && x->min_p <= 1.f)) return fail(c, DTK_ERR_ARG, "%s: min_p must be in [0, 1]", who);
  if (!(x->epsilon_cutoff >= 0.f && x->epsilon_cutoff < 1.f)) return fail(c, DTK_ERR_ARG, "%s: epsilon_cutoff must be in [0, 1)", who);
  return DTK_OK;
}
extern "C++" ExtDev ext_dev(const dtk_sampling_ext* x) {
  ExtDev d{};
  d.qmin = (int64_t)((double)x->min_p * 2147483648.0); d.eps = x->epsilon_cutoff;
  return d;
}

int dtk_set_sampling_ext(dtk_ctx* c, const dtk_sampling_ext* x) {
  if (!c) return DTK_ERR_ARG;
  if (const int rc = ext_check(c, x, "dtk_set_sampling_ext")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const ExtDev dv = ext_dev(x);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(reinterpret_cast<char*>(c->sp) + offsetof(SamplingDev, qmin), &dv, sizeof dv, hipMemcpyHostToDevice));
  c->sampling_ext = *x;
  c->trunc_single = dv.qmin != 0 || dv.eps != 0.f;
  return DTK_OK;
}

int dtk_set_sampling_slot_ext(dtk_ctx* c, int slot, const dtk_sampling_ext* x) {
  if (!c || slot < 0 || slot >= c->nb) return fail(c, DTK_ERR_ARG, "dtk_set_sampling_slot_ext: slot %d of %d", slot, c ? c->nb : 0);
  if (const int rc = ext_check(c, x, "dtk_set_sampling_slot_ext")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const ExtDev dv = ext_dev(x);
  char* dst = reinterpret_cast<char*>(c->sp_b + slot) + offsetof(SamplingDev, qmin);
  if (c->sp_stage) {        // queued behind the slot's dtk_set_sampling_slot upload, from the same staging record
    c->sp_stage[slot].eps = dv.eps; c->sp_stage[slot].qmin = dv.qmin;
    HIPCHK(c, hipMemcpyAsync(dst, &c->sp_stage[slot].qmin, sizeof dv, hipMemcpyHostToDevice, c->stream));
  } else {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, &dv, sizeof dv, hipMemcpyHostToDevice));
  }
  c->slot_trunc[slot] = dv.qmin != 0 || dv.eps != 0.f;
  bool tr = false;
  for (int j = 0; j < c->nb; ++j) tr = tr || c->slot_trunc[j];
  c->trunc_batch = tr;
  return DTK_OK;
}

int dtk_set_sampling(dtk_ctx* c, const dtk_sampling* sp) {
  if (!c) return DTK_ERR_ARG;
  return set_sampling_impl(c, sp, c->sp, c->st, true);
}

int dtk_set_sampling_slot(dtk_ctx* c, int slot, const dtk_sampling* sp) {
  if (!c || slot < 0 || slot >= c->nb) return fail(c, DTK_ERR_ARG, "dtk_set_sampling_slot: slot %d of %d", slot, c ? c->nb : 0);
  return set_sampling_impl(c, sp, c->sp_b + slot, c->st_b + slot, false);
}

// presence / frequency penalty of the sequence the last dtk_set_sampling[_slot] configured (include/dtk.h)
int dtk_set_penalties(dtk_ctx* c, float presence, float frequency, int start) {
  if (!c) return DTK_ERR_ARG;
  if (const int rc = pen_check(c, presence, frequency, start, "dtk_set_penalties")) return rc;
  if (c->launched != c->waited) return fail(c, DTK_ERR_STATE, "dtk_set_penalties: %d decode step(s) are unread", (int)(c->launched - c->waited));
  HIPCHK(c, hipSetDevice(c->device));
  return pen_set(c, 0, presence, frequency, start);
}

int dtk_set_penalties_slot(dtk_ctx* c, int slot, float presence, float frequency, int start) {
  if (!c || slot < 0 || slot >= c->nb) return fail(c, DTK_ERR_ARG, "dtk_set_penalties_slot: slot %d of %d", slot, c ? c->nb : 0);
  if (const int rc = pen_check(c, presence, frequency, start, "dtk_set_penalties_slot")) return rc;
  for (uint64_t q = c->bwaited; q < c->blaunched; ++q)
    if (c->bs_host[q % DTK_MAX_INFLIGHT].active[slot]) return fail(c, DTK_ERR_STATE, "dtk_set_penalties_slot: slot %d is part of an unread step", slot);
  HIPCHK(c, hipSetDevice(c->device));
  return pen_set(c, 1 + slot, presence, frequency, start);
}

// Diagnostic: the count table the next step of the sequence will read (slot -1: the single sequence); zeros while the feature is off
int dtk_token_counts(dtk_ctx* c, int slot, uint16_t* out, int V) {
  if (!c || !out || slot < -1 || slot >= c->nb || V < 1 || V > c->V) return fail(c, DTK_ERR_ARG, "dtk_token_counts: bad argument");
  if (!c->pen_tab) { memset(out, 0, sizeof(uint16_t) * (size_t)V); return DTK_OK; }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, c->pen_tab + (size_t)(slot + 1) * c->pen_stride, sizeof(uint16_t) * (size_t)V, hipMemcpyDeviceToHost));
  return DTK_OK;
}

// DRY of the sequence the last dtk_set_sampling[_slot] configured (include/dtk.h)
int dtk_set_dry(dtk_ctx* c, const dtk_dry* d) {
  if (!c) return DTK_ERR_ARG;
  if (const int rc = dry_check(c, d, c->V, "dtk_set_dry")) return rc;
  if (c->launched != c->waited) return fail(c, DTK_ERR_STATE, "dtk_set_dry: %d decode step(s) are unread", (int)(c->launched - c->waited));
  HIPCHK(c, hipSetDevice(c->device));
  return dry_set(c, 0, d);
}

int dtk_set_dry_slot(dtk_ctx* c, int slot, const dtk_dry* d) {
  if (!c || slot < 0 || slot >= c->nb) return fail(c, DTK_ERR_ARG, "dtk_set_dry_slot: slot %d of %d", slot, c ? c->nb : 0);
  if (const int rc = dry_check(c, d, c->V, "dtk_set_dry_slot")) return rc;
  for (uint64_t q = c->bwaited; q < c->blaunched; ++q)
    if (c->bs_host[q % DTK_MAX_INFLIGHT].active[slot]) return fail(c, DTK_ERR_STATE, "dtk_set_dry_slot: slot %d is part of an unread step", slot);
  HIPCHK(c, hipSetDevice(c->device));
  return dry_set(c, 1 + slot, d);
}

// Diagnostic: the history the next scan of the sequence will read (slot -1: the single sequence): its length, or a negative error; at
// most n_max ids go to ids_out.  0 while the feature is off
int dtk_dry_history(dtk_ctx* c, int slot, int32_t* ids_out, int n_max) {
  if (!c || slot < -1 || slot >= c->nb || n_max < 0 || (n_max > 0 && !ids_out)) return fail(c, DTK_ERR_ARG, "dtk_dry_history: bad argument");
  if (!c->dry_tab) return 0;
  if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, DTK_ERR_HIP, "dtk_dry_history: the stream failed");
  DryLen l{};
  if (hipMemcpy(&l, c->dry_len + (slot + 1), sizeof l, hipMemcpyDeviceToHost) != hipSuccess) return fail(c, DTK_ERR_HIP, "dtk_dry_history: copy failed");
  const int k = l.n < n_max ? l.n : n_max;
  if (k > 0 && hipMemcpy(ids_out, c->dry_hist + (size_t)(slot + 1) * c->Tmax, sizeof(int32_t) * (size_t)k, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(c, DTK_ERR_HIP, "dtk_dry_history: copy failed");
  return l.n;
}

// Diagnostic: the bytes of device and pinned memory the DRY state holds; 0 as long as no sequence of the context ever had a multiplier
int64_t dtk_dry_state_bytes(const dtk_ctx* c) {
  if (!c || !c->dry_tab) return 0;
  const size_t nseq = (size_t)(1 + c->nb), nrec = 1 + DTK_MAX_SLOTS;
  return (int64_t)(nseq * c->dry_stride + 2 * nrec * sizeof(DryDev) + 3 * nseq * c->Tmax * sizeof(int32_t) + 2 * nrec * sizeof(DryLen) +
                   nrec * sizeof(int32_t));
}

// length control / logit bias of the sequence the last dtk_set_sampling[_slot] configured (include/dtk.h)
static int single_idle(dtk_ctx* c, const char* who) {
  if (c->launched != c->waited) return fail(c, DTK_ERR_STATE, "%s: %d decode step(s) are unread", who, (int)(c->launched - c->waited));
  return DTK_OK;
}
static int slot_idle(dtk_ctx* c, int slot, const char* who) {
  for (uint64_t q = c->bwaited; q < c->blaunched; ++q)
    if (c->bs_host[q % DTK_MAX_INFLIGHT].active[slot]) return fail(c, DTK_ERR_STATE, "%s: slot %d is part of an unread step", who, slot);
  return DTK_OK;
}

int dtk_set_length_control(dtk_ctx* c, const dtk_length_ctl* l) {
  if (!c) return DTK_ERR_ARG;
  if (const int rc = len_check(c, l, c->V, "dtk_set_length_control")) return rc;
  if (const int rc = single_idle(c, "dtk_set_length_control")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return len_set(c, 0, l);
}

int dtk_set_length_control_slot(dtk_ctx* c, int slot, const dtk_length_ctl* l) {
  if (!c || slot < 0 || slot >= c->nb) return fail(c, DTK_ERR_ARG, "dtk_set_length_control_slot: slot %d of %d", slot, c ? c->nb : 0);
  if (const int rc = len_check(c, l, c->V, "dtk_set_length_control_slot")) return rc;
  if (const int rc = slot_idle(c, slot, "dtk_set_length_control_slot")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return len_set(c, 1 + slot, l);
}

int dtk_set_logit_bias(dtk_ctx* c, const int32_t* ids, const float* values, int n) {
  if (!c) return DTK_ERR_ARG;
  if (const int rc = bias_check(c, ids, values, n, c->V, "dtk_set_logit_bias")) return rc;
  if (const int rc = single_idle(c, "dtk_set_logit_bias")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return bias_set(c, 0, ids, values, n);
}

int dtk_set_logit_bias_slot(dtk_ctx* c, int slot, const int32_t* ids, const float* values, int n) {
  if (!c || slot < 0 || slot >= c->nb) return fail(c, DTK_ERR_ARG, "dtk_set_logit_bias_slot: slot %d of %d", slot, c ? c->nb : 0);
  if (const int rc = bias_check(c, ids, values, n, c->V, "dtk_set_logit_bias_slot")) return rc;
  if (const int rc = slot_idle(c, slot, "dtk_set_logit_bias_slot")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return bias_set(c, 1 + slot, ids, values, n);
}

// Diagnostic: the dense bias table the sequence's next sampler will read (slot -1: the single sequence) to out[0, V): the number of
// entries != 0, or a negative error; zeros while the feature is off
int dtk_logit_bias_table(dtk_ctx* c, int slot, float* out, int V) {
  if (!c || slot < -1 || slot >= c->nb || !out || V != c->V) return fail(c, DTK_ERR_ARG, "dtk_logit_bias_table: bad argument");
  if (!c->bias_tab) { memset(out, 0, sizeof(float) * (size_t)V); return 0; }
  if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, DTK_ERR_HIP, "dtk_logit_bias_table: the stream failed");
  if (hipMemcpy(out, c->bias_tab + (size_t)(slot + 1) * c->bias_stride, sizeof(float) * (size_t)V, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(c, DTK_ERR_HIP, "dtk_logit_bias_table: copy failed");
  int k = 0;
  for (int i = 0; i < V; ++i) k += out[i] != 0.f;
  return k;
}

// ---- classifier-free guidance: pairs of decoding slots --------------------------------------------------------------------------
static int cfg_find(const dtk_ctx* c, int slot) {      // the pair `slot` belongs to, or -1
  for (int p = 0; p < c->cfg_n; ++p)
    if (c->cfg_pairs[p].cond == slot || c->cfg_pairs[p].uncond == slot) return p;
  return -1;
}
// the device table and the scratch: every buffer on its own, so a call that failed part-way is completed by the next one
static int cfg_alloc(dtk_ctx* c) {
  const size_t np = DTK_MAX_BATCH / 2;
  if (!c->cfg_dev) HIPCHK(c, hipMalloc(&c->cfg_dev, sizeof(CfgPair) * np));
  if (!c->cfg_part) HIPCHK(c, hipMalloc(&c->cfg_part, sizeof(float2) * np * 2 * DTK_CFG_MAX_SLICES));
  if (!c->cfg_lse) { HIPCHK(c, hipMalloc(&c->cfg_lse, sizeof(float2) * np)); HIPCHK(c, hipMemset(c->cfg_lse, 0, sizeof(float2) * np)); }
  if (!c->cfg_forced) { HIPCHK(c, hipMalloc(&c->cfg_forced, sizeof(int32_t) * np)); HIPCHK(c, hipMemset(c->cfg_forced, 0, sizeof(int32_t) * np)); }
  return DTK_OK;
}
// next[0, n) become the pairs, on the host and (where the table exists) on the device; every other entry is unused (cond < 0)
static int cfg_upload(dtk_ctx* c, CfgPair* next, int n) {
  for (int p = n; p < DTK_MAX_BATCH / 2; ++p) next[p] = CfgPair{-1, -1, 1.f, 0};
  if (c->cfg_dev) {
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (no step is in flight; a direct-launch step of before may still read the table)
    HIPCHK(c, hipMemcpy(c->cfg_dev, next, sizeof(CfgPair) * (DTK_MAX_BATCH / 2), hipMemcpyHostToDevice));
  }
  memcpy(c->cfg_pairs, next, sizeof(CfgPair) * (DTK_MAX_BATCH / 2));
  c->cfg_n = n;
  return DTK_OK;
}
int dtk_set_guidance(dtk_ctx* c, int cond_slot, int uncond_slot, float scale) {
  if (!c) return fail(c, DTK_ERR_ARG, "dtk_set_guidance: null context");
  if (c->nb <= 0) return fail(c, DTK_ERR_ARG, "dtk_set_guidance: the context was created without batch slots");
  const int lim = max_decode_slots(c);
  if (cond_slot < 0 || cond_slot >= lim) return fail(c, DTK_ERR_ARG, "dtk_set_guidance: slot %d cannot decode: slots 0..%d of this %d-slot context do", cond_slot, lim - 1, c->nb);
  if (!std::isfinite(scale) || scale < 0.f || scale > 100.f) return fail(c, DTK_ERR_ARG, "dtk_set_guidance: guidance scale %g is not a finite value in [0, 100]", (double)scale);
  const bool dissolve = uncond_slot < 0 || scale == 1.f;
  if (!dissolve) {
    if (uncond_slot >= lim) return fail(c, DTK_ERR_ARG, "dtk_set_guidance: slot %d cannot decode: slots 0..%d of this %d-slot context do", uncond_slot, lim - 1, c->nb);
    if (uncond_slot == cond_slot) return fail(c, DTK_ERR_ARG, "dtk_set_guidance: a pair needs two distinct slots (got %d twice)", cond_slot);
  }
  if (c->blaunched != c->bwaited) return fail(c, DTK_ERR_STATE, "dtk_set_guidance: a batch step is in flight");
  if (c->spec_on) return fail(c, DTK_ERR_STATE, "dtk_set_guidance: slot 0 is speculating (dtk_spec_end first)");
  const int pc = cfg_find(c, cond_slot);
  int n = c->cfg_n;
  CfgPair next[DTK_MAX_BATCH / 2];
  memcpy(next, c->cfg_pairs, sizeof next);
  if (dissolve) {
    if (pc < 0 || next[pc].cond != cond_slot) return DTK_OK;      // heads no pair: nothing to dissolve
    for (int p = pc; p + 1 < n; ++p) next[p] = next[p + 1];
    --n;
  } else {
    const int pu = cfg_find(c, uncond_slot);
    const bool same = pc >= 0 && pc == pu && next[pc].cond == cond_slot && next[pc].uncond == uncond_slot;   // the pair again: a new scale
    if (!same && pc >= 0) return fail(c, DTK_ERR_ARG, "dtk_set_guidance: slot %d is already in the pair (%d, %d)", cond_slot, next[pc].cond, next[pc].uncond);
    if (!same && pu >= 0) return fail(c, DTK_ERR_ARG, "dtk_set_guidance: slot %d is already in the pair (%d, %d)", uncond_slot, next[pu].cond, next[pu].uncond);
    if (same) next[pc].scale = scale;
    else {
      if (n >= DTK_MAX_BATCH / 2) return fail(c, DTK_ERR_ARG, "dtk_set_guidance: at most %d pairs", DTK_MAX_BATCH / 2);
      next[n++] = CfgPair{cond_slot, uncond_slot, scale, 0};
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (n) if (const int rc = cfg_alloc(c)) return rc;
  const int grid_was = cfg_grid(c);
  if (const int rc = cfg_upload(c, next, n)) return rc;
  // the captured steps hold the pair dimension of the grid and whether the kernels run at all.  Standing pairs (dtk_reserve_guidance)
  // that still fit: neither changed, the captures go on reading the table
  if (!c->cfg_res || cfg_grid(c) != grid_was) drop_batch_graphs(c);
  return DTK_OK;
}

int dtk_reserve_guidance(dtk_ctx* c, int n_pairs) {
  if (!c) return fail(c, DTK_ERR_ARG, "dtk_reserve_guidance: null context");
  if (c->nb <= 0) return fail(c, DTK_ERR_ARG, "dtk_reserve_guidance: the context was created without batch slots");
  if (n_pairs < 0 || n_pairs > DTK_MAX_BATCH / 2) return fail(c, DTK_ERR_ARG, "dtk_reserve_guidance: %d pairs is outside 0..%d", n_pairs, DTK_MAX_BATCH / 2);
  if (c->blaunched != c->bwaited) return fail(c, DTK_ERR_STATE, "dtk_reserve_guidance: a batch step is in flight");
  HIPCHK(c, hipSetDevice(c->device));
  if (n_pairs) if (const int rc = cfg_alloc(c)) return rc;
  const int grid_was = cfg_grid(c);
  c->cfg_res = n_pairs;
  CfgPair next[DTK_MAX_BATCH / 2];
  memcpy(next, c->cfg_pairs, sizeof next);
  if (const int rc = cfg_upload(c, next, c->cfg_n)) return rc;
  if (cfg_grid(c) != grid_was) drop_batch_graphs(c);
  if (!cfg_grid(c)) {      // 0 with no live pair: the table goes back (cfg_upload has waited for the stream)
    if (c->cfg_dev) { (void)hipFree(c->cfg_dev); c->cfg_dev = nullptr; }
    if (c->cfg_part) { (void)hipFree(c->cfg_part); c->cfg_part = nullptr; }
    if (c->cfg_lse) { (void)hipFree(c->cfg_lse); c->cfg_lse = nullptr; }
    if (c->cfg_forced) { (void)hipFree(c->cfg_forced); c->cfg_forced = nullptr; }
  }
  return DTK_OK;
}
int64_t dtk_batch_graph_captures(const dtk_ctx* c) { return c ? c->bgraph_captures : 0; }

// diagnostic: the pair `slot` is in.  partner -1 = none (is_cond 0, scale 1, lse NaN); lse_out[2] = (Lc, Lu) of the pair's last step
int dtk_get_guidance(dtk_ctx* c, int slot, int* partner_out, int* is_cond_out, float* scale_out, float* lse_out) {
  if (!c || slot < 0 || slot >= c->nb) return fail(c, DTK_ERR_ARG, "dtk_get_guidance: bad argument");
  const int p = cfg_find(c, slot);
  if (partner_out) *partner_out = p < 0 ? -1 : (c->cfg_pairs[p].cond == slot ? c->cfg_pairs[p].uncond : c->cfg_pairs[p].cond);
  if (is_cond_out) *is_cond_out = p >= 0 && c->cfg_pairs[p].cond == slot;
  if (scale_out) *scale_out = p < 0 ? 1.f : c->cfg_pairs[p].scale;
  if (lse_out) {
    lse_out[0] = lse_out[1] = NAN;
    if (p >= 0) {
      HIPCHK(c, hipSetDevice(c->device));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      HIPCHK(c, hipMemcpy(lse_out, c->cfg_lse + p, sizeof(float2), hipMemcpyDeviceToHost));
    }
  }
  return DTK_OK;
}

int dtk_num_slots(const dtk_ctx* c) { return c ? c->nb : 0; }
int dtk_max_positions(const dtk_ctx* c) { return c ? c->Tmax : 0; }
int dtk_max_decode_slots(const dtk_ctx* c) { return (c && c->nb > 0) ? max_decode_slots(c) : 0; }

// Shared prefixes for k_attn_prefix_g: the active slots grouped by (share_src, share_len) — both properties of the slot alone, so a
// slot's arithmetic never depends on which other slots decode with it — in chunks of 16 (one MFMA column tile), sources in slot
// order.  A source slot that decodes itself is not a member of its forks' groups (that WOULD depend on the others); more than
// DTK_PFX_GROUPS = 64 groups cover the worst case (64 slots that share nothing), so no slot ever falls back because of its company.
// hb->active / share_src / share_len are read; n_groups, group_plus1, pfx_len_of and groups are written (enabled = false: no groups).
extern "C++" void build_prefix_groups(BatchState* hb, const int32_t* active, bool enabled) {
  hb->n_groups = 0;
  for (int j = 0; j < DTK_MAX_BATCH; ++j) { hb->group_plus1[j] = 0; hb->pfx_len_of[j] = 0; }
  if (!enabled) return;
  for (int j = 0; j < DTK_MAX_BATCH && hb->n_groups < DTK_PFX_GROUPS; ++j) {
    if (!active[j] || hb->group_plus1[j] || hb->share_src[j] < 0 || hb->share_len[j] < 4) continue;
    const int src = hb->share_src[j], len = hb->share_len[j];
    PfxGroup* g = nullptr;
    for (int k = j; k < DTK_MAX_BATCH; ++k) {
      if (!active[k] || hb->group_plus1[k] || hb->share_src[k] != src || hb->share_len[k] != len) continue;
      if (!g || g->n == 16) {
        if (hb->n_groups == DTK_PFX_GROUPS) break;
        g = &hb->groups[hb->n_groups++];
        g->src = src; g->len = len; g->n = 0; g->pad = 0;
      }
      g->slot[g->n++] = k;
      hb->group_plus1[k] = hb->n_groups;
      hb->pfx_len_of[k] = len;
    }
  }
  for (int gi = 0; gi < hb->n_groups; ++gi)
    for (int k = hb->groups[gi].n; k < 16; ++k) hb->groups[gi].slot[k] = hb->groups[gi].slot[0];
}

// One batched decode step for the slots with active[slot] != 0 (every one must have been prefilled).
int dtk_decode_batch_launch(dtk_ctx* c, const int32_t* active) {
  if (!c || !active) return fail(c, DTK_ERR_ARG, "dtk_decode_batch_launch: null argument");
  if (c->nb <= 0) return fail(c, DTK_ERR_STATE, "context was created without batch slots");
  if (c->spec_on) return fail(c, DTK_ERR_STATE, "dtk_decode_batch_launch: slot 0 is speculating (dtk_spec_end first)");
  if (c->blaunched - c->bwaited >= DTK_MAX_INFLIGHT) return fail(c, DTK_ERR_STATE, "too many batch steps in flight");
  int n_active = 0;
  for (int j = 0; j < DTK_MAX_BATCH; ++j) {
    if (!active[j]) continue;
    if (j >= max_decode_slots(c)) return fail(c, DTK_ERR_ARG, "slot %d cannot decode: slots 0..%d of this %d-slot context do", j, max_decode_slots(c) - 1, c->nb);
    const SeqHost& sh = c->bseq[(size_t)j];
    if (!sh.have_logits) return fail(c, DTK_ERR_STATE, "slot %d: decode before prefill", j);
    if (sh.host_next_pos >= c->Tmax) return fail(c, DTK_ERR_RANGE, "slot %d: context length %d reached max_positions", j, sh.host_next_pos);
    ++n_active;
  }
  if (!n_active) return fail(c, DTK_ERR_ARG, "no active slot");
  for (int p = 0; p < c->cfg_n; ++p) {      // a guided pair decodes together or not at all
    const CfgPair& gp = c->cfg_pairs[p];
    if ((active[gp.cond] != 0) != (active[gp.uncond] != 0))
      return fail(c, DTK_ERR_ARG, "dtk_decode_batch_launch: guided pair (%d, %d): slot %d is active without slot %d (dtk_set_guidance pairs them; both or neither take part in a step)",
                  gp.cond, gp.uncond, active[gp.cond] ? gp.cond : gp.uncond, active[gp.cond] ? gp.uncond : gp.cond);
    const bool fc = c->bseq[(size_t)gp.cond].forced_pending >= 0, fu = c->bseq[(size_t)gp.uncond].forced_pending >= 0;
    if (active[gp.cond] && fc != fu)      // one slot would forward its last prompt token while the other one samples: the rows would not belong together
      return fail(c, DTK_ERR_ARG, "dtk_decode_batch_launch: guided pair (%d, %d): slot %d was resumed (dtk_resume_slot) and forwards its last prompt token in this step, slot %d does not; resume both slots or prefill both",
                  gp.cond, gp.uncond, fc ? gp.cond : gp.uncond, fc ? gp.uncond : gp.cond);
  }
  HIPCHK(c, hipSetDevice(c->device));
  ensure_tiled_weights(c);
  BatchState* hb = c->bs_host + (c->blaunched % DTK_MAX_INFLIGHT);
  for (int j = 0; j < DTK_MAX_BATCH; ++j) {
    hb->active[j] = active[j] ? 1 : 0;
    const bool sh_ok = c->share_reads && j < c->nb && c->bseq[(size_t)j].share_src >= 0;
    hb->share_src[j] = sh_ok ? c->bseq[(size_t)j].share_src : -1;
    hb->share_len[j] = sh_ok ? c->bseq[(size_t)j].share_len : 0;
    hb->kv8_from[j] = c->kv8 && j < c->nb ? c->bseq[(size_t)j].kv8_from : 0;
  }
  hb->step = (int32_t)(c->blaunched % DTK_MAX_INFLIGHT);
  build_prefix_groups(hb, active, c->prefix_mfma && !mv_family(c));
  int hi = 0;
  for (int j = 0; j < DTK_MAX_BATCH; ++j) if (active[j]) hi = j;
  c->nt_step = hi < 16 ? 1 : (hi < 32 ? 2 : 4);      // column tiles this step needs (per-column results do not depend on it)
  c->mv_step = mv_family(c) ? (hi < 1 ? 1 : (hi < 2 ? 2 : 4)) : 0;   // vectors of a multi-vector step (per-slot results do not depend on it)
  HIPCHK(c, hipMemcpyAsync(c->bs_dev, hb, sizeof(BatchState), hipMemcpyHostToDevice, c->stream));
  if (c->use_graph) {
    int rc = ensure_batch_graph(c);
    if (rc) return rc;
    HIPCHK(c, hipGraphLaunch(c->bgraph_exec[step_graph_index(c)], c->stream));
  } else {
    c->launch_refused = false;
    if (c->mv_step) batch_step_launches_mv(c); else batch_step_launches(c);
    if (c->launch_refused || dtk_lds_attr_error(c->device))
      return fail(c, DTK_ERR_STATE, c->launch_refused ? "batched step: a projection's shape has no kernel in its family (nothing launched for it)"
                                                      : "batched step: raising a kernel's dynamic-LDS limit failed (hipFuncSetAttribute, see stderr)");
    HIPCHK(c, hipMemcpyAsync(c->tokb_host, c->tokb_dev, sizeof(int64_t) * TOKB_WORDS, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, copy_lp_ring(c, true));
  }
  HIPCHK(c, hipEventRecord(c->bstep_done[c->blaunched % DTK_MAX_INFLIGHT], c->stream));
  c->stats.last_batch_step_slots = (uint32_t)(c->mv_step ? c->mv_step : 16 * c->nt_step);
  c->stats.last_batch_step_fp8_mfma = (!c->mv_step && mx_step(c)) ? 1u : 0u;
  c->blaunched++;
  c->stats.decode_steps++;
  for (int j = 0; j < DTK_MAX_BATCH; ++j)
    if (active[j]) { c->bseq[(size_t)j].host_next_pos++; c->bseq[(size_t)j].cached_ids.push_back(-1); c->bseq[(size_t)j].forced_pending = -1; }
  return DTK_OK;
}

// tokens_out[DTK_MAX_BATCH]: the token sampled for every slot that was active in the oldest un-read step (-1 otherwise)
// one TopRec + its logsumexp -> DTK_MAX_TOP (id, logprob = z - lse) pairs; entries >= k (and all of a NULL record): -1, NaN
static void top_unpack(const TopRec* r, const float* lse, int k, int32_t* ids_out, float* lp_out) {
  for (int i = 0; i < DTK_MAX_TOP; ++i) { ids_out[i] = -1; lp_out[i] = NAN; }
  if (!r) return;
  const float e = *(const volatile float*)lse;
  for (int i = 0; i < k; ++i) {
    ids_out[i] = ((const volatile int32_t*)r->id)[i];
    lp_out[i] = ((const volatile float*)r->z)[i] - e;
  }
}

static int decode_batch_wait_impl(dtk_ctx* c, int64_t* tokens_out, float* logprob_out, float* sample_logprob_out,
                                  int32_t* top_ids_out = nullptr, float* top_logprob_out = nullptr) {
  if (c->spec_on) return fail(c, DTK_ERR_STATE, "dtk_decode_batch_wait: the steps in flight are speculative ones (dtk_spec_wait)");
  if (c->bwaited >= c->blaunched) return fail(c, DTK_ERR_STATE, "no batch step in flight");
  HIPCHK(c, hipSetDevice(c->device));
  const uint64_t k = c->bwaited;
  const int ring = (int)(k % DTK_MAX_INFLIGHT);
  HIPCHK(c, hipEventSynchronize(c->bstep_done[ring]));
  const uint32_t dev_err = (uint32_t)((volatile int64_t*)c->tokb_host)[TOKB_ERR];
  if (dev_err) {      // sticky: the tokens of this and every later step cannot be trusted
    c->stats.device_errors = dev_err;
    c->bwaited++;
    return fail(c, DTK_ERR_HIP, "%u in-kernel hand-off waits expired (LDS-ring GEMVs): the step's results are invalid; re-create the context", dev_err);
  }
  const BatchState* hb = c->bs_host + ring;
  // how many steps were launched after step k for each slot (their cached ids are still -1)
  for (int j = 0; j < DTK_MAX_BATCH; ++j) {
    tokens_out[j] = -1;
    if (logprob_out) logprob_out[j] = sample_logprob_out[j] = NAN;
    if (top_ids_out) top_unpack(nullptr, nullptr, 0, top_ids_out + (size_t)j * DTK_MAX_TOP, top_logprob_out + (size_t)j * DTK_MAX_TOP);
    if (!hb->active[j]) continue;
    const int64_t tok = ((volatile int64_t*)c->tokb_host)[(size_t)ring * DTK_MAX_BATCH + j];
    tokens_out[j] = tok;
    if (logprob_out) {
      const volatile float* lp = (volatile float*)(c->lpb_host + (size_t)ring * DTK_MAX_BATCH + j);
      logprob_out[j] = lp[0]; sample_logprob_out[j] = lp[1];
    }
    if (top_ids_out)
      top_unpack(c->topb_host + (size_t)ring * DTK_MAX_BATCH + j, c->lseb_host + (size_t)ring * DTK_MAX_BATCH + j, c->top_logprobs,
                 top_ids_out + (size_t)j * DTK_MAX_TOP, top_logprob_out + (size_t)j * DTK_MAX_TOP);
    SeqHost& sh = c->bseq[(size_t)j];
    size_t later = 0;
    for (uint64_t q = k + 1; q < c->blaunched; ++q) later += c->bs_host[q % DTK_MAX_INFLIGHT].active[j] ? 1 : 0;
    if (sh.cached_ids.size() > later) sh.cached_ids[sh.cached_ids.size() - 1 - later] = tok;
  }
  c->bwaited++;
  return DTK_OK;
}

int dtk_decode_batch_wait(dtk_ctx* c, int64_t* tokens_out) {
  if (!c || !tokens_out) return fail(c, DTK_ERR_ARG, "dtk_decode_batch_wait: null argument");
  return decode_batch_wait_impl(c, tokens_out, nullptr, nullptr);
}

// dtk_decode_batch_wait + the (logprob, sample_logprob) of every token it returns (NaN where tokens_out is -1, and for a forced token)
int dtk_decode_batch_wait_lp(dtk_ctx* c, int64_t* tokens_out, float* logprob_out, float* sample_logprob_out) {
  if (!c || !tokens_out || !logprob_out || !sample_logprob_out) return fail(c, DTK_ERR_ARG, "dtk_decode_batch_wait_lp: null argument");
  if (!c->logprobs) return fail(c, DTK_ERR_ARG, "dtk_decode_batch_wait_lp: the context does not compute log-probabilities (dtk_set_option \"logprobs\", 1)");
  return decode_batch_wait_impl(c, tokens_out, logprob_out, sample_logprob_out);
}

// dtk_decode_batch_wait_lp + every slot's top-k alternatives, [DTK_MAX_BATCH][DTK_MAX_TOP] (dtk_set_option "top_logprobs")
int dtk_decode_batch_wait_top(dtk_ctx* c, int64_t* tokens_out, float* logprob_out, float* sample_logprob_out, int32_t* top_ids_out,
                              float* top_logprob_out) {
  if (!c || !tokens_out || !logprob_out || !sample_logprob_out || !top_ids_out || !top_logprob_out)
    return fail(c, DTK_ERR_ARG, "dtk_decode_batch_wait_top: null argument");
  if (!c->logprobs || !c->top_logprobs)
    return fail(c, DTK_ERR_ARG, "dtk_decode_batch_wait_top: the context does not compute top-k alternatives (dtk_set_option \"logprobs\", 1 and \"top_logprobs\", k)");
  return decode_batch_wait_impl(c, tokens_out, logprob_out, sample_logprob_out, top_ids_out, top_logprob_out);
}

// ---- prompt-lookup speculative decoding of slot 0 (include/dtk.h)
static int spec_alloc(dtk_ctx* c) {
  if (c->spec_mem) return DTK_OK;
  size_t off = 0;
  auto room = [&](size_t bytes) { const size_t at = off; off = align_up(off + bytes, 256); return at; };
  const size_t o_sd = room(sizeof(SpecDev)), o_hist = room((size_t)c->Tmax * 4), o_tab = room((size_t)c->Tmax * 4);
  const size_t o_st = room(4 * sizeof(DecState)), o_sp = room(4 * sizeof(SamplingDev)), o_bs = room(sizeof(BatchState));
  HIPCHK(c, hipMalloc((void**)&c->spec_mem, off));
  c->spec_sd = reinterpret_cast<SpecDev*>(c->spec_mem + o_sd);
  c->spec_hist = reinterpret_cast<int32_t*>(c->spec_mem + o_hist);
  c->spec_table = reinterpret_cast<int32_t*>(c->spec_mem + o_tab);
  c->spec_st = reinterpret_cast<DecState*>(c->spec_mem + o_st);
  c->spec_sp = reinterpret_cast<SamplingDev*>(c->spec_mem + o_sp);
  c->spec_bs = reinterpret_cast<BatchState*>(c->spec_mem + o_bs);
  return DTK_OK;
}

int dtk_spec_begin(dtk_ctx* c, int K, int max_ngram, int source) {
  if (!c) return fail(c, DTK_ERR_ARG, "dtk_spec_begin: null context");
  if (K < 1 || K > 3) return fail(c, DTK_ERR_ARG, "dtk_spec_begin: %d drafts per step is outside 1..3", K);
  if (max_ngram < 1 || max_ngram > DTK_SPEC_MAX_NGRAM) return fail(c, DTK_ERR_ARG, "dtk_spec_begin: max_ngram %d is outside 1..%d", max_ngram, DTK_SPEC_MAX_NGRAM);
  if (source != DTK_SPEC_LOOKUP && source != DTK_SPEC_TABLE) return fail(c, DTK_ERR_ARG, "dtk_spec_begin: draft source %d (DTK_SPEC_LOOKUP | DTK_SPEC_TABLE)", source);
  if (!mv_family(c)) return fail(c, DTK_ERR_STATE, "dtk_spec_begin: the context is outside the multi-vector family (2..5 batch slots): the verify pass is the multi-vector step");
  if (max_decode_slots(c) < K + 1) return fail(c, DTK_ERR_ARG, "dtk_spec_begin: %d drafts per step need %d decoding slots, the context has %d", K, K + 1, max_decode_slots(c));
  if (c->kv8) return fail(c, DTK_ERR_STATE, "dtk_spec_begin: kv_format mxfp8 (the vectors of a step share slot 0's rows: bf16 contexts only)");
  if (c->spec_on) return fail(c, DTK_ERR_STATE, "dtk_spec_begin: slot 0 is speculating already");
  if (c->engine_holds.load() > 0) return fail(c, DTK_ERR_STATE, "dtk_spec_begin: a batch engine holds sequences in the context's slots");
  if (c->cfg_n) return fail(c, DTK_ERR_STATE, "dtk_spec_begin: the context has a guided pair (dtk_set_guidance)");
  if (c->top_logprobs) return fail(c, DTK_ERR_STATE, "dtk_spec_begin: top_logprobs is on (its records are per slot and step)");
  for (int j = 0; j < c->nb; ++j) {      // their tables depend on the position (and any slot's values change the sampler the step launches)
    if (pen_on(c, 1 + j)) return fail(c, DTK_ERR_STATE, "dtk_spec_begin: slot %d has a presence / frequency penalty", j);
    if (dry_on(c, 1 + j)) return fail(c, DTK_ERR_STATE, "dtk_spec_begin: slot %d has DRY", j);
    if (len_on(c, 1 + j)) return fail(c, DTK_ERR_STATE, "dtk_spec_begin: slot %d has length control or a logit bias", j);
  }
  if (c->blaunched != c->bwaited) return fail(c, DTK_ERR_STATE, "dtk_spec_begin: a batch step is in flight");
  SeqHost& sh = c->bseq[0];
  if (!sh.have_logits) return fail(c, DTK_ERR_STATE, "dtk_spec_begin: slot 0 has no pending logits (prefill it first)");
  if (sh.forced_pending >= 0) return fail(c, DTK_ERR_STATE, "dtk_spec_begin: slot 0 was resumed and forwards its last prompt token first (prefill it, or decode that step)");
  const int n = (int)sh.cached_ids.size();
  if (n < 1 || n != sh.host_next_pos || n > c->Tmax) return fail(c, DTK_ERR_STATE, "dtk_spec_begin: slot 0 holds %d ids at length %d", n, sh.host_next_pos);
  std::vector<int32_t> h((size_t)c->Tmax, 0), none((size_t)c->Tmax, -1);
  for (int i = 0; i < n; ++i) {
    if (sh.cached_ids[(size_t)i] < 0) return fail(c, DTK_ERR_STATE, "dtk_spec_begin: slot 0 has un-read tokens");
    h[(size_t)i] = (int32_t)sh.cached_ids[(size_t)i];
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (const int rc = spec_alloc(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->spec_hist, h.data(), (size_t)c->Tmax * 4, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->spec_table, none.data(), (size_t)c->Tmax * 4, hipMemcpyHostToDevice));
  std::vector<BatchState> hb(1);
  memset(hb.data(), 0, sizeof(BatchState));
  hb[0].active[0] = 1;                     // only vector 0 has a pending row: slot 0's own
  for (int j = 0; j < DTK_MAX_BATCH; ++j) hb[0].share_src[j] = -1;
  hb[0].step = (int32_t)(c->blaunched % DTK_MAX_INFLIGHT);
  HIPCHK(c, hipMemcpy(c->spec_bs, hb.data(), sizeof(BatchState), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->spec_st, c->st_b, sizeof(DecState), hipMemcpyDeviceToDevice));
  for (int j = 0; j < 4; ++j) HIPCHK(c, hipMemcpy(c->spec_sp + j, c->sp_b, sizeof(SamplingDev), hipMemcpyDeviceToDevice));
  SpecDev sd{};
  sd.drafts[0] = h[(size_t)n - 1]; sd.drafts[1] = sd.drafts[2] = sd.drafts[3] = -1; sd.n_live = 1;
  sd.K = K; sd.NV = K + 1; sd.max_ngram = max_ngram; sd.use_table = source == DTK_SPEC_TABLE ? 1 : 0;
  sd.corpus_len = c->spec_corpus_len; sd.corpus = c->spec_corpus; sd.corpus_best = c->spec_corpus_best;      // (the step counters start at 0)
  HIPCHK(c, hipMemcpy(c->spec_sd, &sd, sizeof sd, hipMemcpyHostToDevice));
  for (int j = 1; j <= K; ++j) c->bseq[(size_t)j].have_logits = false;      // their logits rows and residual rows become the vectors'; their KV stays
  c->spec_K = K; c->spec_src = source; c->spec_nv = K + 1;      // (the n-gram size lives in spec_sd alone)
  c->spec_known_pos = n;
  c->spec_on = true;
  return DTK_OK;
}

int dtk_spec_set_drafts(dtk_ctx* c, const int32_t* table, int n) {
  if (!c || (!table && n > 0) || n < 0) return fail(c, DTK_ERR_ARG, "dtk_spec_set_drafts: bad argument");
  if (!c->spec_on || c->spec_src != DTK_SPEC_TABLE) return fail(c, DTK_ERR_STATE, "dtk_spec_set_drafts: slot 0 is not speculating from a table (dtk_spec_begin(.., DTK_SPEC_TABLE))");
  if (n > c->Tmax) return fail(c, DTK_ERR_ARG, "dtk_spec_set_drafts: %d positions exceed max_positions %d", n, c->Tmax);
  if (c->blaunched != c->bwaited) return fail(c, DTK_ERR_STATE, "dtk_spec_set_drafts: a step is in flight");
  std::vector<int32_t> t((size_t)c->Tmax, -1);
  for (int i = 0; i < n; ++i) {
    if (table[i] < -1 || table[i] >= c->V) return fail(c, DTK_ERR_ARG, "dtk_spec_set_drafts: id %d at position %d (-1 or a token id)", table[i], i);
    t[(size_t)i] = table[i];
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->spec_table, t.data(), (size_t)c->Tmax * 4, hipMemcpyHostToDevice));
  return DTK_OK;
}

// the corpus of earlier programs, the lookup's second draft source (include/dtk.h).  Pointer and length reach the kernels through
// spec_sd, so the captured steps serve every corpus; only the change between none and some changes what a step launches
int dtk_spec_set_corpus(dtk_ctx* c, const int32_t* ids, int n) {
  if (!c || (!ids && n > 0) || n < 0) return fail(c, DTK_ERR_ARG, "dtk_spec_set_corpus: bad argument");
  if (n > DTK_SPEC_CORPUS_MAX) return fail(c, DTK_ERR_RANGE, "dtk_spec_set_corpus: a corpus of %d entries exceeds DTK_SPEC_CORPUS_MAX = %d", n, DTK_SPEC_CORPUS_MAX);
  if (!mv_family(c)) return fail(c, DTK_ERR_STATE, "dtk_spec_set_corpus: the context is outside the multi-vector family (2..5 batch slots): it has no speculative step");
  if (c->spec_on && c->blaunched != c->bwaited) return fail(c, DTK_ERR_STATE, "dtk_spec_set_corpus: a speculative step is in flight");
  for (int i = 0; i < n; ++i)
    if (ids[i] >= c->V) return fail(c, DTK_ERR_ARG, "dtk_spec_set_corpus: corpus id %d at entry %d (a token id below %d, or a negative separator)", ids[i], i, c->V);
  if (n == 0 && c->spec_corpus_len == 0) return DTK_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (n > 0 && !c->spec_corpus) {
    const size_t ids_bytes = (size_t)DTK_SPEC_CORPUS_MAX * sizeof(int32_t);
    HIPCHK(c, hipMalloc((void**)&c->spec_corpus, ids_bytes + DTK_SPEC_CORPUS_BLOCKS * sizeof(unsigned long long)));
    c->spec_corpus_best = reinterpret_cast<unsigned long long*>(reinterpret_cast<unsigned char*>(c->spec_corpus) + ids_bytes);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n > 0) HIPCHK(c, hipMemcpy(c->spec_corpus, ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
  if ((n > 0) != (c->spec_corpus_len > 0)) {      // a step with k_spec_corpus <-> a step without it: the two captures go (one re-capture each)
    for (int i = 0; i < 2; ++i) {
      if (c->sgraph_exec[i]) { (void)hipGraphExecDestroy(c->sgraph_exec[i]); c->sgraph_exec[i] = nullptr; }
      if (c->sgraph[i]) { (void)hipGraphDestroy(c->sgraph[i]); c->sgraph[i] = nullptr; }
      c->sgraph_ready[i] = false;
    }
  }
  c->spec_corpus_len = n;
  if (c->spec_sd) {      // (a context that has not speculated yet has no record: dtk_spec_begin writes these three)
    const int32_t len32 = n;
    HIPCHK(c, hipMemcpy(&c->spec_sd->corpus_len, &len32, sizeof len32, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(&c->spec_sd->corpus, &c->spec_corpus, sizeof c->spec_corpus, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(&c->spec_sd->corpus_best, &c->spec_corpus_best, sizeof c->spec_corpus_best, hipMemcpyHostToDevice));
  }
  return DTK_OK;
}

int dtk_spec_corpus_len(const dtk_ctx* c) { return c ? c->spec_corpus_len : 0; }

int dtk_spec_counters(dtk_ctx* c, int64_t* out) {
  if (!c || !out) return fail(c, DTK_ERR_ARG, "dtk_spec_counters: bad argument");
  if (c->spec_on && c->blaunched != c->bwaited) return fail(c, DTK_ERR_STATE, "dtk_spec_counters: a step is in flight");
  out[0] = out[1] = out[2] = 0;
  if (!c->spec_sd) return DTK_OK;      // the context has never speculated
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  long long steps[3];
  HIPCHK(c, hipMemcpy(steps, c->spec_sd->steps, sizeof steps, hipMemcpyDeviceToHost));
  out[0] = steps[DTK_SPEC_FROM_HISTORY]; out[1] = steps[DTK_SPEC_FROM_CORPUS]; out[2] = steps[DTK_SPEC_FROM_NONE];
  return DTK_OK;
}

static int ensure_spec_graph(dtk_ctx* c, int gi) {      // c->spec_step and c->mv_step are set
  if (c->bgraph_trunc != c->trunc_batch) { drop_batch_graphs(c); c->bgraph_trunc = c->trunc_batch; }
  if (c->sgraph_ready[gi]) return DTK_OK;
  HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  c->launch_refused = false;
  batch_step_launches_mv(c);
  HIPCHK(c, hipMemcpyAsync(c->tokb_host, c->tokb_dev, sizeof(int64_t) * TOKB_WORDS, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, copy_lp_ring(c, true));
  HIPCHK(c, hipStreamEndCapture(c->stream, &c->sgraph[gi]));
  if (c->launch_refused || dtk_lds_attr_error(c->device)) {       // an incomplete step must never be replayed
    (void)hipGraphDestroy(c->sgraph[gi]); c->sgraph[gi] = nullptr;
    return fail(c, DTK_ERR_STATE, c->launch_refused ? "speculative step: a projection's shape has no kernel in its family (nothing launched for it)"
                                                    : "speculative step: raising a kernel's dynamic-LDS limit failed (hipFuncSetAttribute, see stderr)");
  }
  HIPCHK(c, hipGraphInstantiate(&c->sgraph_exec[gi], c->sgraph[gi], nullptr, nullptr, 0));
  c->sgraph_ready[gi] = true;
  c->bgraph_captures++;
  return DTK_OK;
}

static int spec_launch_impl(dtk_ctx* c) {
  const int gi = c->spec_nv <= 2 ? 0 : 1;
  if (c->use_graph) {
    if (const int rc = ensure_spec_graph(c, gi)) return rc;
    HIPCHK(c, hipGraphLaunch(c->sgraph_exec[gi], c->stream));
  } else {
    c->launch_refused = false;
    batch_step_launches_mv(c);
    if (c->launch_refused || dtk_lds_attr_error(c->device))
      return fail(c, DTK_ERR_STATE, c->launch_refused ? "speculative step: a projection's shape has no kernel in its family (nothing launched for it)"
                                                      : "speculative step: raising a kernel's dynamic-LDS limit failed (hipFuncSetAttribute, see stderr)");
    HIPCHK(c, hipMemcpyAsync(c->tokb_host, c->tokb_dev, sizeof(int64_t) * TOKB_WORDS, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, copy_lp_ring(c, true));
  }
  return DTK_OK;
}

int dtk_spec_launch(dtk_ctx* c) {
  if (!c) return fail(c, DTK_ERR_ARG, "dtk_spec_launch: null context");
  if (!c->spec_on) return fail(c, DTK_ERR_STATE, "dtk_spec_launch: slot 0 is not speculating (dtk_spec_begin)");
  const int inflight = (int)(c->blaunched - c->bwaited);
  if (inflight >= DTK_MAX_INFLIGHT) return fail(c, DTK_ERR_STATE, "too many batch steps in flight");
  // the position this step starts at is known only once the steps in flight have been read: each of them accepts at most 4 tokens
  if (c->spec_known_pos + 4 * inflight >= c->Tmax)
    return fail(c, DTK_ERR_RANGE, "slot 0: context length %d (+ at most %d of %d steps in flight) reached max_positions", c->spec_known_pos, 4 * inflight, inflight);
  HIPCHK(c, hipSetDevice(c->device));
  ensure_tiled_weights(c);
  BatchState* hb = c->bs_host + (c->blaunched % DTK_MAX_INFLIGHT);      // the host's record of the step: which slots it keeps busy
  for (int j = 0; j < DTK_MAX_BATCH; ++j) hb->active[j] = j <= c->spec_K ? 1 : 0;
  hb->step = (int32_t)(c->blaunched % DTK_MAX_INFLIGHT);
  c->nt_step = 1;
  c->mv_step = c->spec_nv <= 2 ? 2 : 4;
  c->spec_step = true;
  const int rc = spec_launch_impl(c);
  c->spec_step = false;
  if (rc) return rc;
  HIPCHK(c, hipEventRecord(c->bstep_done[c->blaunched % DTK_MAX_INFLIGHT], c->stream));
  c->stats.last_batch_step_slots = (uint32_t)c->mv_step;
  c->stats.last_batch_step_fp8_mfma = 0u;
  c->blaunched++;
  c->stats.decode_steps++;
  return DTK_OK;
}

int dtk_spec_wait(dtk_ctx* c, int64_t* tokens_out, int* n_out, float* logprob_out, float* sample_logprob_out) {
  if (!c || !tokens_out || !n_out || (logprob_out == nullptr) != (sample_logprob_out == nullptr)) return fail(c, DTK_ERR_ARG, "dtk_spec_wait: bad argument");
  if (logprob_out && !c->logprobs) return fail(c, DTK_ERR_ARG, "dtk_spec_wait: the context does not compute log-probabilities (dtk_set_option \"logprobs\", 1)");
  if (!c->spec_on) return fail(c, DTK_ERR_STATE, "dtk_spec_wait: slot 0 is not speculating (dtk_spec_begin)");
  if (c->bwaited >= c->blaunched) return fail(c, DTK_ERR_STATE, "no batch step in flight");
  HIPCHK(c, hipSetDevice(c->device));
  const int ring = (int)(c->bwaited % DTK_MAX_INFLIGHT);
  HIPCHK(c, hipEventSynchronize(c->bstep_done[ring]));
  const volatile int64_t* rec = (volatile int64_t*)c->tokb_host + (size_t)ring * DTK_MAX_BATCH;
  const int64_t cnt = rec[DTK_SPEC_COUNT_AT];
  c->bwaited++;
  if (cnt < 1 || cnt > c->spec_nv) return fail(c, DTK_ERR_HIP, "dtk_spec_wait: the step reports %lld accepted tokens (1..%d)", (long long)cnt, c->spec_nv);
  SeqHost& sh = c->bseq[0];
  for (int i = 0; i < 4; ++i) {
    tokens_out[i] = i < cnt ? rec[i] : -1;
    if (logprob_out) {
      const volatile float* lp = (volatile float*)(c->lpb_host + (size_t)ring * DTK_MAX_BATCH + i);
      logprob_out[i] = i < cnt ? lp[0] : NAN; sample_logprob_out[i] = i < cnt ? lp[1] : NAN;
    }
    if (i < cnt) sh.cached_ids.push_back(tokens_out[i]);
  }
  sh.host_next_pos += (int)cnt;
  c->spec_known_pos += (int)cnt;
  *n_out = (int)cnt;
  return DTK_OK;
}

int dtk_spec_end(dtk_ctx* c, int keep_len) {
  if (!c) return fail(c, DTK_ERR_ARG, "dtk_spec_end: null context");
  if (!c->spec_on) return fail(c, DTK_ERR_STATE, "dtk_spec_end: slot 0 is not speculating (dtk_spec_begin)");
  while (c->bwaited < c->blaunched) {      // the steps still in flight: their tokens are the sequence's too (keep_len says which stay)
    int64_t toks[4]; int n = 0;
    if (dtk_spec_wait(c, toks, &n, nullptr, nullptr)) { c->bwaited = c->blaunched; c->spec_on = false; c->bseq[0].have_logits = false; return DTK_ERR_HIP; }
  }
  SeqHost& sh = c->bseq[0];
  if (keep_len < 1 || (size_t)keep_len > sh.cached_ids.size())
    return fail(c, DTK_ERR_ARG, "dtk_spec_end: keep_len %d, slot 0 holds %zu ids", keep_len, sh.cached_ids.size());
  sh.cached_ids.resize((size_t)keep_len);
  sh.host_next_pos = keep_len;
  sh.have_logits = false;                  // the pending rows belong to positions that may have been dropped: the next prefill recomputes one
  if (sh.share_len > keep_len) sh.share_len = keep_len;
  if (sh.share_len <= 0) { sh.share_src = -1; sh.share_len = 0; }
  sh.last_reuse_start = keep_len;
  c->spec_on = false;
  return DTK_OK;
}

// Copy the KV of the first n_tokens positions of slot src into slot dst (SURVEY §8 f1 / the proposed
// dtk_kv_fork): rollouts that share a prefix (always: the 243 image tokens) reuse its KV bit for bit instead
// of re-running ViT + prefill.  dst then needs a dtk_prefill_slot(..., DTK_PREFILL_REUSE_PREFIX) of the full
// prompt, which only processes what lies beyond the common prefix (at least the last token).
int dtk_kv_fork(dtk_ctx* c, int src, int dst, int n_tokens) {
  if (!c || src < 0 || dst < 0 || src >= c->nb || dst >= c->nb || src == dst)
    return fail(c, DTK_ERR_ARG, "dtk_kv_fork: bad slots %d -> %d of %d", src, dst, c ? c->nb : 0);
  if (c->spec_on) return fail(c, DTK_ERR_STATE, "dtk_kv_fork: slot 0 is speculating (dtk_spec_end first)");
  SeqHost& a = c->bseq[(size_t)src];
  if (n_tokens < 1 || (size_t)n_tokens > a.cached_ids.size() || n_tokens > c->Tmax)
    return fail(c, DTK_ERR_ARG, "dtk_kv_fork: %d tokens but slot %d holds %zu", n_tokens, src, a.cached_ids.size());
  for (int i = 0; i < n_tokens; ++i)
    if (a.cached_ids[(size_t)i] < 0) return fail(c, DTK_ERR_STATE, "dtk_kv_fork: source has un-read tokens");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t pitch = (size_t)c->Tmax * 128 * 2;           // one (layer, k|v, head) plane
  const size_t rows = (size_t)c->L * 2 * c->KVH;
  HIPCHK(c, hipMemcpy2DAsync(c->kvb + (size_t)dst * c->kv_slot_stride, pitch, c->kvb + (size_t)src * c->kv_slot_stride, pitch,
                             (size_t)n_tokens * 128 * 2, rows, hipMemcpyDeviceToDevice, c->stream));
  SeqHost& b = c->bseq[(size_t)dst];
  for (int j = 0; j < c->nb; ++j)          // whoever read its prefix from dst must stop: dst is being overwritten
    if (c->bseq[(size_t)j].share_src == dst) { c->bseq[(size_t)j].share_src = -1; c->bseq[(size_t)j].share_len = 0; }
  // dst now holds a bit-identical copy of src[0, n): its attention may read those rows from src (or from src's own
  // source when src itself is a fork covering them), so all forks of one prefix stream the same memory
  if (a.share_src >= 0 && a.share_src != dst && n_tokens <= a.share_len) { b.share_src = a.share_src; b.share_len = n_tokens; }
  else { b.share_src = src; b.share_len = n_tokens; }
  b.cached_ids.assign(a.cached_ids.begin(), a.cached_ids.begin() + n_tokens);
  b.forced_pending = -1;
  if (const int rc = pen_rebuild(c, 1 + dst, b.cached_ids.data(), n_tokens)) return rc;
  b.cached_with_image = a.cached_with_image;
  b.image_key = a.image_key;
  b.host_next_pos = n_tokens;
  b.kv8_from = n_tokens;                   // nothing of the shadow is copied: the destination's rows [0, n) are bf16 rows
  b.have_logits = false;
  // a fork of the WHOLE source sequence also inherits its next-token logits: the destination can decode at
  // once (a rollout from the MCTS root needs no prefill at all).  The source must not have decoded since its
  // prefill (its logits buffer would belong to a later position).
  if ((size_t)n_tokens == a.cached_ids.size() && a.have_logits && a.host_next_pos == n_tokens) {
    HIPCHK(c, hipMemcpyAsync(c->logits_b + (size_t)dst * c->V, c->logits_b + (size_t)src * c->V, (size_t)c->V * 4,
                             hipMemcpyDeviceToDevice, c->stream));
    DecState& st0 = c->st_stage[dst];             // pinned per-slot record: queued behind the step in flight, no drain
    st0 = DecState{};
    st0.pos = n_tokens - 1; st0.next_pos = n_tokens; st0.token = (int32_t)a.cached_ids[(size_t)n_tokens - 1]; st0.draw = 0;
    HIPCHK(c, hipMemcpyAsync(c->st_b + dst, &st0, sizeof st0, hipMemcpyHostToDevice, c->stream));
    b.have_logits = true;
  }
  return DTK_OK;
}

// kv_format "mxfp8": the slot's boundary — its rows [from, length) were written by decode steps and are read from the MXFP8 shadow.
int dtk_kv8_info(dtk_ctx* c, int slot, int* from_out) {
  if (!c || !from_out || slot < 0 || slot >= c->nb) return fail(c, DTK_ERR_ARG, "dtk_kv8_info: bad argument");
  if (!c->kv8) return fail(c, DTK_ERR_STATE, "dtk_kv8_info: the context keeps bf16 key/value rows only (kv_format bf16)");
  *from_out = c->bseq[(size_t)slot].kv8_from;
  return DTK_OK;
}

// Diagnostic: rows [row0, row0 + nrows) of one layer's K (which = 0) or V (1) planes of a decoding slot, every kv head: the shadow's
// codes [KVH][nrows][128] and scales [KVH][nrows][4] and the bf16 rows beside them [KVH][nrows][128] (any of the three may be NULL).
// Waits for the launched steps first.
int dtk_read_kv8(dtk_ctx* c, int slot, int layer, int which, int row0, int nrows, uint8_t* codes_out, uint8_t* scales_out, uint16_t* bf16_out) {
  if (!c || slot < 0 || slot >= c->nb || layer < 0 || layer >= c->L || which < 0 || which > 1 || row0 < 0 || nrows < 1 || row0 + nrows > c->Tmax)
    return fail(c, DTK_ERR_ARG, "dtk_read_kv8: bad argument");
  if (!c->kv8) return fail(c, DTK_ERR_STATE, "dtk_read_kv8: the context keeps bf16 key/value rows only (kv_format bf16)");
  if (slot >= c->kv8_slots) return fail(c, DTK_ERR_ARG, "dtk_read_kv8: slot %d never decodes and has no shadow rows (slots 0..%d do)", slot, c->kv8_slots - 1);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t plane = ((size_t)slot * c->L * 2 + (size_t)layer * 2 + which) * c->KVH * c->Tmax;      // rows before this (slot, layer, k|v) plane
  const size_t first = plane + row0;
  if (codes_out) HIPCHK(c, hipMemcpy2D(codes_out, (size_t)nrows * 128, c->kv8c + first * 128, (size_t)c->Tmax * 128, (size_t)nrows * 128, c->KVH, hipMemcpyDeviceToHost));
  if (scales_out) HIPCHK(c, hipMemcpy2D(scales_out, (size_t)nrows * 4, c->kv8s + first * 4, (size_t)c->Tmax * 4, (size_t)nrows * 4, c->KVH, hipMemcpyDeviceToHost));
  if (bf16_out) HIPCHK(c, hipMemcpy2D(bf16_out, (size_t)nrows * 256, c->kvb + first * 128, (size_t)c->Tmax * 256, (size_t)nrows * 256, c->KVH, hipMemcpyDeviceToHost));
  return DTK_OK;
}

// Longest common prefix of `ids` with what slot's KV cache holds (prefilled AND decoded tokens), under the rules of
// DTK_PREFILL_REUSE_PREFIX: an image prompt only matches a cache computed with the same image key.  The engine uses it to give
// a returning MCTS tree the slot that still holds its previous rollout.
int dtk_slot_lcp(dtk_ctx* c, int slot, const int64_t* ids, int T, uint64_t image_key, int* lcp_out) {
  if (!c || !ids || !lcp_out || T < 1 || slot < 0 || slot >= c->nb) return fail(c, DTK_ERR_ARG, "dtk_slot_lcp: bad argument");
  const SeqHost& sh = c->bseq[(size_t)slot];
  int img_count = 0;
  for (int t = 0; t < T; ++t) img_count += ids[t] == c->cfg.image_token_id;
  const bool has_img = img_count > 0;
  const bool same_image = !has_img ? !sh.cached_with_image : (sh.cached_with_image && image_key != 0 && sh.image_key == image_key);
  int n = 0;
  if (same_image) {
    const int lim = (int)std::min<size_t>(sh.cached_ids.size(), (size_t)T);
    while (n < lim && sh.cached_ids[(size_t)n] == ids[n]) ++n;
  }
  *lcp_out = n;
  return DTK_OK;
}

// Diagnostic: the token ids slot's cache is known to hold (-1 = a decoded token whose step has not been read yet); returns the
// number of ids written (at most n_max).
int dtk_slot_cached_ids(dtk_ctx* c, int slot, int64_t* out, int n_max) {
  if (!c || !out || slot < 0 || slot >= c->nb || n_max < 0) return -1;
  const SeqHost& sh = c->bseq[(size_t)slot];
  const int n = (int)std::min<size_t>(sh.cached_ids.size(), (size_t)n_max);
  for (int i = 0; i < n; ++i) out[i] = sh.cached_ids[(size_t)i];
  return n;
}

// Resume decoding in place: the slot's cache already holds ids[0, T-1) (dtk_slot_lcp >= T - 1) — typically the path to an MCTS
// node inside the slot's own previous rollout.  No prefill: the context is cut back to T - 1 tokens and the NEXT batched step
// forwards ids[T-1] for this slot instead of sampling (DecState.force_plus1), returning ids[T-1] as that step's token; the step
// after it samples the first new token (draw 0: begin-suppress applies there).  The rows [0, T-1) stay as they were written
// (by the prefill GEMMs and / or the decode kernels of the earlier sequence), like any DTK_PREFILL_REUSE_PREFIX hit.
int dtk_resume_slot(dtk_ctx* c, int slot, const int64_t* ids, int T, uint64_t image_key) {
  if (!c || !ids || T < 2 || slot < 0 || slot >= c->nb) return fail(c, DTK_ERR_ARG, "dtk_resume_slot: bad argument");
  if (T > c->Tmax) return fail(c, DTK_ERR_RANGE, "prompt of %d tokens exceeds max_positions %d", T, c->Tmax);
  if (c->spec_on) return fail(c, DTK_ERR_STATE, "dtk_resume_slot: slot 0 is speculating (dtk_spec_end first)");
  if (ids[T - 1] == c->cfg.image_token_id) return fail(c, DTK_ERR_ARG, "dtk_resume_slot: the last prompt token is an image position (its input is a patch feature, not an embedding)");
  int lcp = 0;
  const int rc = dtk_slot_lcp(c, slot, ids, T, image_key, &lcp);
  if (rc) return rc;
  if (lcp < T - 1) return fail(c, DTK_ERR_STATE, "dtk_resume_slot: slot %d holds %d of the %d prompt tokens (needs %d)", slot, lcp, T, T - 1);
  for (uint64_t q = c->bwaited; q < c->blaunched; ++q)
    if (c->bs_host[q % DTK_MAX_INFLIGHT].active[slot]) return fail(c, DTK_ERR_STATE, "dtk_resume_slot: slot %d is part of a step in flight", slot);
  HIPCHK(c, hipSetDevice(c->device));
  SeqHost& sh = c->bseq[(size_t)slot];
  for (int j = 0; j < c->nb; ++j) {        // forks that read rows >= T - 1 from this slot would see them overwritten
    SeqHost& o = c->bseq[(size_t)j];
    if (o.share_src == slot && o.share_len > T - 1) { o.share_src = -1; o.share_len = 0; }
  }
  if (sh.share_len > T - 1) sh.share_len = T - 1;
  if (sh.share_len <= 0) { sh.share_src = -1; sh.share_len = 0; }
  sh.cached_ids.resize((size_t)T - 1);
  sh.forced_pending = ids[T - 1];          // (a dtk_set_penalties_slot before the step that forwards it counts it too)
  if (const int rc = pen_rebuild(c, 1 + slot, ids, T)) return rc;      // with the forced ids[T-1]: the step that forwards it counts nothing
  sh.host_next_pos = T - 1;
  sh.kv8_from = std::min(sh.kv8_from, T - 1);      // the rows this slot decoded earlier and keeps stay MXFP8 rows
  sh.have_logits = true;                   // "may decode": the first step does not read the logits buffer
  sh.last_reuse_start = T - 1;
  DecState& st0 = c->st_stage[slot];
  st0 = DecState{};
  st0.pos = T - 2; st0.next_pos = T - 1; st0.token = (int32_t)ids[T - 2]; st0.draw = 0; st0.force_plus1 = (int32_t)ids[T - 1] + 1;
  HIPCHK(c, hipMemcpyAsync(c->st_b + slot, &st0, sizeof st0, hipMemcpyHostToDevice, c->stream));   // ordered behind the step in flight
  return DTK_OK;
}

int dtk_get_logits_slot(dtk_ctx* c, int slot, float* out) {
  if (!c || !out || slot < 0 || slot >= c->nb) return fail(c, DTK_ERR_ARG, "dtk_get_logits_slot: bad argument");
  if (!c->bseq[(size_t)slot].have_logits) return fail(c, DTK_ERR_STATE, "no logits yet");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, c->logits_b + (size_t)slot * c->V, (size_t)c->V * 4, hipMemcpyDeviceToHost));
  return DTK_OK;
}

int dtk_context_len_slot(const dtk_ctx* c, int slot) {
  return (c && slot >= 0 && slot < c->nb) ? c->bseq[(size_t)slot].host_next_pos : -1;
}

int dtk_set_graph_mode(dtk_ctx* c, int enabled) {
  if (!c) return DTK_ERR_ARG;
  c->use_graph = enabled == 1;
  c->probe = enabled == 2;   // 2: plain launches with HIP-event probe around the gate/up GEMV
  if (c->probe && c->stats.probe_event_pair_ms == 0.0) {
    // what an event pair costs with NOTHING between the two records (timestamp packets): part of every probe interval
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double sum = 0.0; int n = 0;
    for (int i = 0; i < 40; ++i) {
      HIPCHK(c, hipEventRecord(c->probe_a, c->stream));
      HIPCHK(c, hipEventRecord(c->probe_b, c->stream));
      HIPCHK(c, hipEventSynchronize(c->probe_b));
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, c->probe_a, c->probe_b) == hipSuccess && i >= 8) { sum += ms; ++n; }
    }
    if (n) c->stats.probe_event_pair_ms = sum / n;
  }
  return DTK_OK;
}

int dtk_decode_launch(dtk_ctx* c) {
  if (!c) return DTK_ERR_ARG;
  if (!c->seq0.have_logits) return fail(c, DTK_ERR_STATE, "dtk_decode before dtk_prefill");
  if (c->launched - c->waited >= DTK_MAX_INFLIGHT) return fail(c, DTK_ERR_STATE, "too many decode steps in flight");
  if (c->seq0.host_next_pos >= c->Tmax) return fail(c, DTK_ERR_RANGE, "context length %d reached max_positions", c->seq0.host_next_pos);
  HIPCHK(c, hipSetDevice(c->device));
  ensure_fp8_weights(c);
  if (int rc = ensure_w13(c)) return rc;
  if (c->use_graph) {
    int rc = ensure_graph(c);
    if (rc) return rc;
    const bool short_ctx = c->seq0.host_next_pos < c->attn_full_max;
    HIPCHK(c, hipGraphLaunch(short_ctx ? c->graph_short_exec : c->graph_exec, c->stream));
  } else {
    if (c->probe && c->launched > c->waited) HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->probe && c->probe_pending) {  // read the previous step's pair before re-recording it
      float ms = 0.f;
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if (hipEventElapsedTime(&ms, c->probe_a, c->probe_b) == hipSuccess) {
        c->stats.probe_kernel_ms_sum += ms;
        c->stats.probe_kernel_launches++;
      }
      c->probe_pending = false;
    }
    decode_step_launches(c, c->probe != 0, c->seq0.host_next_pos < c->attn_full_max);
    if (c->probe) c->probe_pending = true;
    HIPCHK(c, hipMemcpyAsync(c->tok_ring_host, c->tok_ring_dev, sizeof(int64_t) * DTK_MAX_INFLIGHT, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, copy_lp_ring(c, false));
  }
  HIPCHK(c, hipEventRecord(c->step_done[c->launched % DTK_MAX_INFLIGHT], c->stream));
  c->launched++;
  c->seq0.host_next_pos++;
  c->stats.decode_steps++;
  c->seq0.cached_ids.push_back(-1);  // filled in by dtk_decode_wait
  return DTK_OK;
}

static int decode_wait_impl(dtk_ctx* c, int64_t* token_out, float* lp_out, int32_t* top_ids_out = nullptr, float* top_logprob_out = nullptr) {
  if (c->waited >= c->launched) return fail(c, DTK_ERR_STATE, "no decode step in flight");
  HIPCHK(c, hipSetDevice(c->device));
  const uint64_t k = c->waited;
  HIPCHK(c, hipEventSynchronize(c->step_done[k % DTK_MAX_INFLIGHT]));
  // the ring slot of draw k is rewritten only by draw k + DTK_MAX_INFLIGHT, which cannot have
  // been launched yet; later copies of the whole ring rewrite it with the same value
  const int64_t tok = ((volatile int64_t*)c->tok_ring_host)[k % DTK_MAX_INFLIGHT];
  *token_out = tok;
  if (lp_out) {
    const volatile float* lp = (volatile float*)(c->lp_ring_host + k % DTK_MAX_INFLIGHT);
    lp_out[0] = lp[0]; lp_out[1] = lp[1];
  }
  if (top_ids_out)
    top_unpack(c->top_ring_host + k % DTK_MAX_INFLIGHT, c->lse_ring_host + k % DTK_MAX_INFLIGHT, c->top_logprobs, top_ids_out, top_logprob_out);
  const size_t idx = c->seq0.cached_ids.size() - (size_t)(c->launched - k);
  c->seq0.cached_ids[idx] = tok;
  c->waited++;
  return DTK_OK;
}

int dtk_decode_wait(dtk_ctx* c, int64_t* token_out) {
  if (!c || !token_out) return fail(c, DTK_ERR_ARG, "dtk_decode_wait: null argument");
  return decode_wait_impl(c, token_out, nullptr);
}

// dtk_decode_wait + lp_out[2] = (logprob, sample_logprob) of the token
int dtk_decode_wait_lp(dtk_ctx* c, int64_t* token_out, float* lp_out) {
  if (!c || !token_out || !lp_out) return fail(c, DTK_ERR_ARG, "dtk_decode_wait_lp: null argument");
  if (!c->logprobs) return fail(c, DTK_ERR_ARG, "dtk_decode_wait_lp: the context does not compute log-probabilities (dtk_set_option \"logprobs\", 1)");
  return decode_wait_impl(c, token_out, lp_out);
}

// dtk_decode_wait_lp + the top-k alternatives of the logits the token was sampled from, DTK_MAX_TOP entries each (dtk_set_option "top_logprobs")
int dtk_decode_wait_top(dtk_ctx* c, int64_t* token_out, float* lp_out, int32_t* top_ids_out, float* top_logprob_out) {
  if (!c || !token_out || !lp_out || !top_ids_out || !top_logprob_out) return fail(c, DTK_ERR_ARG, "dtk_decode_wait_top: null argument");
  if (!c->logprobs || !c->top_logprobs)
    return fail(c, DTK_ERR_ARG, "dtk_decode_wait_top: the context does not compute top-k alternatives (dtk_set_option \"logprobs\", 1 and \"top_logprobs\", k)");
  return decode_wait_impl(c, token_out, lp_out, top_ids_out, top_logprob_out);
}

int dtk_decode(dtk_ctx* c, int64_t* token_out) {
  int rc = dtk_decode_launch(c);
  if (rc) return rc;
  return dtk_decode_wait(c, token_out);
}

int dtk_get_logits(dtk_ctx* c, float* out) {
  if (!c || !out) return fail(c, DTK_ERR_ARG, "dtk_get_logits: null argument");
  if (!c->seq0.have_logits) return fail(c, DTK_ERR_STATE, "no logits yet");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, c->logits, (size_t)c->V * 4, hipMemcpyDeviceToHost));
  return DTK_OK;
}

int dtk_context_len(const dtk_ctx* c) { return c ? c->seq0.host_next_pos : -1; }

int dtk_synchronize(dtk_ctx* c) {
  if (!c) return DTK_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return DTK_OK;
}

int dtk_get_stats(dtk_ctx* c, dtk_stats* out) {
  if (!c || !out) return DTK_ERR_ARG;
  *out = c->stats;
  return DTK_OK;
}

// In-situ microbenchmark of one decode GEMV role over all layers (distinct weights per launch,
// so nothing is served from the 256 MB Infinity Cache): avg microseconds per launch via HIP events.
// role: 0 qkv, 1 o_proj, 2 gate/up, 3 down, 4 lm_head.  Clobbers the decode state.
// variant | 0x800 (with 0xff): the role streams the context's weight FORMAT as a decode step does (fp8 rows + row scales, MXFP4 codes +
// block scales, lm_head fp8 in both); without the bit the bf16 masters are streamed whatever the format (what the bit-less callers measure).
int dtk_bench_gemv(dtk_ctx* c, int role, int variant, int reps, float* avg_us) {
  if (!c || !avg_us || reps < 1) return fail(c, DTK_ERR_ARG, "dtk_bench_gemv: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (role < 0 || role > 4) return fail(c, DTK_ERR_ARG, "dtk_bench_gemv: role %d (0 qkv, 1 o_proj, 2 gate/up, 3 down, 4 lm_head)", role);
  const bool same_layer = (variant & 0x100) != 0;  // every launch re-reads layer 0 (Infinity Cache probe)
  const int plain = (variant >> 9) & 3;            // 0x200: same weights through PRO_COPY + EPI_STORE; 0x400: PRO_RMSNORM + EPI_STORE
  const bool fmt = (variant & 0x800) != 0;
  // bf16 contexts with option "w13": 0xff streams what the step streams - the 13-bit planes of the roles that have them, in the step's shape
  // (so the time goes with dtk_stats.probe_kernel_bytes).  0x2000 | 0xff: the bf16 rows in the step's bf16 kernel whatever "w13" says.
  // 0x1000 | shape: the planes in that 13-bit shape; a role whose matrices the step keeps as bf16 rows (o_proj) is packed for this call only.
  const bool b13 = (variant & 0x1000) != 0, raw16 = (variant & 0x2000) != 0;
  if (b13 && (fmt || raw16 || plain || same_layer || c->wfmt != 0 || !c->w13 || (variant & 0xff) == 0xff))
    return fail(c, DTK_ERR_ARG, "dtk_bench_gemv: 0x1000 | shape (13-bit planes) needs a bf16 context with w13 = 1, a shape number and no other flag");
  if (raw16 && ((variant & 0xff) != 0xff || plain || fmt)) return fail(c, DTK_ERR_ARG, "dtk_bench_gemv: 0x2000 (bf16 rows) goes with variant 0xff only");
  const bool step13 = w13_on(c) && !raw16 && !plain && (variant & 0xff) == 0xff;      // the shipped kernel on what the step streams
  struct Tmp13 { std::vector<uint8_t*> p, h; ~Tmp13() { for (auto x : p) if (x) (void)hipFree(x); for (auto x : h) if (x) (void)hipFree(x); } } tmp13;
  if (b13 || step13) { if (int rc = ensure_w13(c)) return rc; }
  if (b13) {
    for (int l = 0; l < c->L && role != 4; ++l) {
      const LayerW& w = c->layers[l];
      const uint8_t* p = role == 0 ? w.p13_wqkv : (role == 1 ? w.p13_wo : (role == 2 ? w.p13_wgu : w.p13_wdown));
      if (p) continue;
      if (role != 1) return fail(c, DTK_ERR_STATE, "dtk_bench_gemv: role %d has no 13-bit planes in layer %d (an unpackable row, or a bf16 fold no 13-bit shape has)", role, l);
      if (!c->w13_bad) HIPCHK(c, hipMalloc((void**)&c->w13_bad, sizeof(unsigned)));
      uint8_t *pp = nullptr, *hh = nullptr;         // o_proj: planes of this call's own
      HIPCHK(c, hipMalloc((void**)&pp, (size_t)c->d * w13_row_bytes(c->d)));
      tmp13.p.push_back(pp);
      HIPCHK(c, hipMalloc((void**)&hh, (size_t)c->d));
      tmp13.h.push_back(hh);
      unsigned bad = 0;
      HIPCHK(c, hipMemsetAsync(c->w13_bad, 0, sizeof(unsigned), s));
      launch_pack_w13_rows(w.wo, pp, hh, c->w13_bad, c->d, c->d, !c->w13_nz, s);
      HIPCHK(c, hipMemcpyAsync(&bad, c->w13_bad, sizeof(unsigned), hipMemcpyDeviceToHost, s));
      HIPCHK(c, hipStreamSynchronize(s));
      if (bad) return fail(c, DTK_ERR_STATE, "dtk_bench_gemv: o_proj of layer %d has %u unpackable row(s)", l, bad);
    }
    if (role == 4 && !c->p13_lm_head) return fail(c, DTK_ERR_STATE, "dtk_bench_gemv: lm_head has no 13-bit planes");
  }
  if (fmt && ((variant & 0xff) != 0xff || plain))   // the numbered variants and the plain probes are bf16 instantiations
    return fail(c, DTK_ERR_ARG, "dtk_bench_gemv: 0x800 (the context's weight format) goes with variant 0xff only");
  if (fmt) ensure_fp8_weights(c);
  variant &= 0xff;
  const bool shipped = variant == 0xff;            // 0xff: whatever launch_gemv picks for this role and model (the kernel a decode step runs)
  if (b13) {
    const int pro = (role == 1 || role == 3) ? PRO_COPY : PRO_RMSNORM;
    const int epi = role == 0 ? EPI_QKV : (role == 2 ? EPI_SWIGLU : (role == 4 ? EPI_LOGITS : EPI_RESID));
    if (!gemv_w13_has(pro, epi, variant)) return fail(c, DTK_ERR_ARG, "dtk_bench_gemv: no 13-bit shape %d for role %d", variant, role);
  }
  auto launch = [&](int pro, int epi, const GemvArgs& g) {
    if (b13) launch_gemv_w13_variant(pro, epi, variant, g, s);
    else if (shipped) launch_gemv(pro, epi, g, s);
    else launch_gemv_variant(pro, epi, variant, g, s);
  };
  auto one_pass = [&]() {
    for (int l = 0; l < c->L; ++l) {
      const LayerW& w = c->layers[same_layer ? 0 : l];
      GemvArgs g{};
      if (plain) {   // cost of the fused prologue / epilogue = full role - this
        g.eps = c->cfg.rms_eps; g.y = c->GU;
        if (role == 0) { g.W = w.wqkv; g.N = c->d + 2 * c->KVH * c->hd; g.K = c->d; g.x = c->x; g.norm_w = w.ln1; }
        else if (role == 1) { g.W = w.wo; g.N = c->d; g.K = c->d; g.x = c->attn_out; g.norm_w = w.ln1; }
        else if (role == 2) { g.W = w.wgu; g.N = 2 * c->ff; g.K = c->d; g.x = c->x; g.norm_w = w.ln2; }
        else if (role == 3) { g.W = w.wdown; g.N = c->d; g.K = c->ff; g.x = c->act; g.norm_w = w.ln2; }
        else { g.W = c->lm_head; g.N = c->V; g.K = c->d; g.x = c->x; g.norm_w = c->final_norm; }
        launch_gemv_variant(plain == 2 ? PRO_RMSNORM : PRO_COPY, EPI_STORE, variant, g, s);
        continue;
      }
      g.eps = c->cfg.rms_eps; g.st = c->st; g.T_max = c->Tmax; g.d = c->d; g.ff = c->ff; g.H = c->H; g.KVH = c->KVH; g.hd = c->hd;
      g.rope_cos = c->rope_cos; g.rope_sin = c->rope_sin; g.pm = c->pm; g.pl = c->pl; g.po = c->po; g.S = c->S;
      if (fmt) {
        if (role == 0) { g.W8 = w.q_wqkv; g.wscale = w.s_wqkv; g.W4 = w.f4_wqkv; g.S4 = w.e4_wqkv; }
        else if (role == 1) { g.W8 = w.q_wo; g.wscale = w.s_wo; g.W4 = w.f4_wo; g.S4 = w.e4_wo; }
        else if (role == 2) { g.W8 = w.q_wgu; g.wscale = w.s_wgu; g.W4 = w.f4_wgu; g.S4 = w.e4_wgu; }
        else if (role == 3) { g.W8 = w.q_wdown; g.wscale = w.s_wdown; g.W4 = w.f4_wdown; g.S4 = w.e4_wdown; }
        else { g.W8 = c->q_lm_head; g.wscale = c->s_lm_head; }
      }
      if (b13 || step13) {
        if (role == 0) { g.Wp = w.p13_wqkv; g.Wh = w.h13_wqkv; }
        else if (role == 1) { g.Wp = w.p13_wo; g.Wh = w.h13_wo; if (!g.Wp && b13) { g.Wp = tmp13.p[(size_t)l]; g.Wh = tmp13.h[(size_t)l]; } }
        else if (role == 2) { g.Wp = w.p13_wgu; g.Wh = w.h13_wgu; }
        else if (role == 3) { g.Wp = w.p13_wdown; g.Wh = w.h13_wdown; }
        else { g.Wp = c->p13_lm_head; g.Wh = c->h13_lm_head; }
      }
      if (role == 0) { g.W = w.wqkv; g.N = c->d + 2 * c->KVH * c->hd; g.K = c->d; g.x = c->x; g.norm_w = w.ln1; g.q_out = c->q; g.kcache = kcache(c, l); g.vcache = vcache(c, l); launch(PRO_RMSNORM, EPI_QKV, g); }
      else if (role == 1) { g.W = w.wo; g.N = c->d; g.K = c->d; g.x = c->attn_out; g.y = c->q; launch(PRO_COPY, EPI_RESID, g); }
      else if (role == 2) { g.W = w.wgu; g.N = 2 * c->ff; g.K = c->d; g.x = c->x; g.norm_w = w.ln2; g.y = c->act; launch(PRO_RMSNORM, EPI_SWIGLU, g); }
      else if (role == 3) { g.W = w.wdown; g.N = c->d; g.K = c->ff; g.x = c->act; g.y = c->q; launch(PRO_COPY, EPI_RESID, g); }
      else { g.W = c->lm_head; g.N = c->V; g.K = c->d; g.x = c->x; g.norm_w = c->final_norm; g.logits = c->logits; launch(PRO_RMSNORM, EPI_LOGITS, g); }
    }
  };
  one_pass();  // warm-up (code objects, clocks)
  HIPCHK(c, hipEventRecord(c->ev_a, s));
  for (int r = 0; r < reps; ++r) one_pass();
  HIPCHK(c, hipEventRecord(c->ev_b, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, c->ev_a, c->ev_b));
  *avg_us = ms * 1e3f / (float)(reps * c->L);
  c->seq0.have_logits = false;
  return DTK_OK;
}

// Runtime options (tests / tuning): "attn_full_max" = contexts below this use the one-block-per-head
// decode attention (0 = always split-K); "attn_combine" = 0 consumer | 1 in-kernel | 2 own kernel.
// tools/bench_cfg.py: what the guidance launches of a step cost on this context's own pairs, rows and step state (HIP events around `reps`
// back-to-back launches): avg_us[0] = k_cfg_lse + k_cfg_mix, avg_us[1] = k_cfg_follow.  The pending rows of the conditional slots are
// mixed `reps` times over: prefill the pairs again before decoding on
int dtk_bench_cfg(dtk_ctx* c, int reps, float* avg_us) {
  if (!c || !avg_us || reps < 1 || reps > 64) return fail(c, DTK_ERR_ARG, "dtk_bench_cfg: bad argument (1 <= reps <= 64)");
  if (!c->cfg_n) return fail(c, DTK_ERR_STATE, "dtk_bench_cfg: the context has no guided pair (dtk_set_guidance)");
  if (c->blaunched != c->bwaited) return fail(c, DTK_ERR_STATE, "dtk_bench_cfg: a batch step is in flight");
  HIPCHK(c, hipSetDevice(c->device));
  SampleArgs sa;
  sa.logits = c->logits_b; sa.V = c->V; sa.logits_stride = c->V; sa.bs = c->bs_dev; sa.st = c->st_b; sa.x = c->xb; sa.d = c->d;
  sa.tok_ring = c->tokb_dev; sa.ring = DTK_MAX_INFLIGHT;
  sa.lp_ring = c->logprobs ? c->lpb_dev : nullptr; sa.lse_ring = (c->logprobs && c->top_logprobs) ? c->lseb_dev : nullptr;
  for (int which = 0; which < 2; ++which) {
    for (int i = 0; i < 3; ++i) { if (which) follow_launch(c, sa); else guidance_launch(c, sa); }      // warm-up
    HIPCHK(c, hipEventRecord(c->probe_a, c->stream));
    for (int i = 0; i < reps; ++i) { if (which) follow_launch(c, sa); else guidance_launch(c, sa); }
    HIPCHK(c, hipEventRecord(c->probe_b, c->stream));
    HIPCHK(c, hipEventSynchronize(c->probe_b));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->probe_a, c->probe_b));
    avg_us[which] = ms * 1000.f / (float)reps;
  }
  return DTK_OK;
}

// tools/bench_spec.py: HIP events around reps back-to-back launches of the speculative step's two own kernels on the sequence's state
int dtk_bench_spec(dtk_ctx* c, int reps, float* avg_us) {
  if (!c || !avg_us || reps < 1 || reps > 64) return fail(c, DTK_ERR_ARG, "dtk_bench_spec: bad argument (1 <= reps <= 64)");
  if (!c->spec_on) return fail(c, DTK_ERR_STATE, "dtk_bench_spec: slot 0 is not speculating (dtk_spec_begin)");
  if (c->blaunched != c->bwaited) return fail(c, DTK_ERR_STATE, "dtk_bench_spec: a step is in flight");
  HIPCHK(c, hipSetDevice(c->device));
  SpecArgs sv;
  sv.sd = c->spec_sd; sv.hist = c->spec_hist; sv.table = c->spec_table; sv.K = 0; sv.max_ngram = 0; sv.NV = 0; sv.T_max = c->Tmax; sv.V = c->V;
  sv.st_true = c->st_b; sv.st_vec = c->spec_st; sv.bs = c->spec_bs; sv.tok_ring = c->tokb_dev; sv.ring = DTK_MAX_INFLIGHT;
  sv.embed = c->embed; sv.x = c->xb; sv.d = c->d;
  const bool corpus = c->spec_corpus_len > 0;      // the step's third kernel, as a step launches it
  for (int i = 0; i < 3; ++i) { launch_spec_accept(sv, c->stream); if (corpus) launch_spec_corpus(sv, c->stream); launch_spec_draft(sv, c->stream); }      // warm-up
  HIPCHK(c, hipEventRecord(c->probe_a, c->stream));
  for (int i = 0; i < reps; ++i) { launch_spec_accept(sv, c->stream); if (corpus) launch_spec_corpus(sv, c->stream); launch_spec_draft(sv, c->stream); }
  HIPCHK(c, hipEventRecord(c->probe_b, c->stream));
  HIPCHK(c, hipEventSynchronize(c->probe_b));
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, c->probe_a, c->probe_b));
  *avg_us = ms * 1000.f / (float)reps;
  // the pairs re-read stale token records and moved the position (never beyond max_positions): the sequence is only good for dtk_spec_end
  const uint32_t ring_was = (uint32_t)(c->blaunched % DTK_MAX_INFLIGHT);
  HIPCHK(c, hipMemcpy(&c->spec_bs->step, &ring_was, sizeof ring_was, hipMemcpyHostToDevice));
  return DTK_OK;
}

int dtk_set_option(dtk_ctx* c, const char* name, int value) {
  if (!c || !name) return DTK_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!strcmp(name, "attn_full_max")) c->attn_full_max = value;
  else if (!strcmp(name, "w13")) {     // bf16 contexts: the single-sequence step streams the 13-bit planes of its weight rows (w13.h; same results)
    if (value != 0 && value != 1) return fail(c, DTK_ERR_ARG, "w13 must be 0 or 1");
    if (value != c->w13) {
      if (c->launched != c->waited) return fail(c, DTK_ERR_STATE, "w13: %d single-sequence decode step(s) are unread", (int)(c->launched - c->waited));
      c->w13 = value; drop_graph(c);
      if (!value) { w13_free(c); w13_set_stats(c); }
      set_weight_bytes(c);
    }
  }
  else if (!strcmp(name, "w13_nz")) {  // 1: rows without a zero code take the short decode (w13.h: W13_ZROW); 0: the packer flags every row (same results; tools/bench_w13.py)
    if (value != 0 && value != 1) return fail(c, DTK_ERR_ARG, "w13_nz must be 0 or 1");
    if (value != c->w13_nz) {
      if (c->launched != c->waited) return fail(c, DTK_ERR_STATE, "w13_nz: %d single-sequence decode step(s) are unread", (int)(c->launched - c->waited));
      c->w13_nz = value;
      if (c->w13_ready) { c->w13_ready = false; drop_graph(c); }   // the planes' row bytes are written again before the next single-sequence step
    }
  }
  else if (!strcmp(name, "logprobs")) {    // every sampled token comes with (logprob, sample_logprob): the LP sampler instantiations + one more D2H copy per step
    if (value != 0 && value != 1) return fail(c, DTK_ERR_ARG, "logprobs must be 0 or 1");
    if (value == 0 && c->top_logprobs) return fail(c, DTK_ERR_STATE, "logprobs: top_logprobs = %d needs it (set \"top_logprobs\" to 0 first)", c->top_logprobs);
    if ((value != 0) != (c->logprobs != 0)) {
      if (c->blaunched != c->bwaited) return fail(c, DTK_ERR_STATE, "logprobs: a batch step is in flight");
      if (c->engine_holds.load() > 0) return fail(c, DTK_ERR_STATE, "logprobs: an engine holds %d sequence(s) in this context's slots", c->engine_holds.load());
      // (their ring entries were written under the other setting; dtk_set_sampling / dtk_prefill start the single sequence afresh)
      if (c->launched != c->waited) return fail(c, DTK_ERR_STATE, "logprobs: %d single-sequence decode step(s) are unread", (int)(c->launched - c->waited));
      c->logprobs = value; drop_graph(c); drop_batch_graphs(c);
    }
  }
  else if (!strcmp(name, "top_logprobs")) {     // + the k most likely tokens of every step's logits: k_top_logits in front of the sampler + two more D2H copies per step
    if (value < 0 || value > DTK_MAX_TOP) return fail(c, DTK_ERR_ARG, "top_logprobs must be 0 .. %d", DTK_MAX_TOP);
    if (value > c->V) return fail(c, DTK_ERR_ARG, "top_logprobs = %d exceeds the vocabulary (%d)", value, c->V);
    if (value != 0 && !c->logprobs) return fail(c, DTK_ERR_STATE, "top_logprobs needs logprobs = 1 (dtk_set_option \"logprobs\", 1 first)");
    if (value != c->top_logprobs) {
      if (c->blaunched != c->bwaited) return fail(c, DTK_ERR_STATE, "top_logprobs: a batch step is in flight");
      if (c->engine_holds.load() > 0) return fail(c, DTK_ERR_STATE, "top_logprobs: an engine holds %d sequence(s) in this context's slots", c->engine_holds.load());
      if (c->launched != c->waited) return fail(c, DTK_ERR_STATE, "top_logprobs: %d single-sequence decode step(s) are unread", (int)(c->launched - c->waited));
      if (value) {      // every buffer on its own: a call that failed part-way is completed by the next one
        const size_t n1 = DTK_MAX_INFLIGHT, nb = c->nb > 0 ? (size_t)DTK_MAX_INFLIGHT * DTK_MAX_BATCH : 0;
        if (!c->top_ring_dev) { HIPCHK(c, hipMalloc(&c->top_ring_dev, sizeof(TopRec) * n1)); HIPCHK(c, hipMemset(c->top_ring_dev, 0, sizeof(TopRec) * n1)); }
        if (!c->lse_ring_dev) { HIPCHK(c, hipMalloc(&c->lse_ring_dev, sizeof(float) * n1)); HIPCHK(c, hipMemset(c->lse_ring_dev, 0, sizeof(float) * n1)); }
        if (!c->top_ring_host) HIPCHK(c, hipHostMalloc((void**)&c->top_ring_host, sizeof(TopRec) * n1, hipHostMallocDefault));
        if (!c->lse_ring_host) HIPCHK(c, hipHostMalloc((void**)&c->lse_ring_host, sizeof(float) * n1, hipHostMallocDefault));
        if (nb && !c->topb_dev) { HIPCHK(c, hipMalloc(&c->topb_dev, sizeof(TopRec) * nb)); HIPCHK(c, hipMemset(c->topb_dev, 0, sizeof(TopRec) * nb)); }
        if (nb && !c->lseb_dev) { HIPCHK(c, hipMalloc(&c->lseb_dev, sizeof(float) * nb)); HIPCHK(c, hipMemset(c->lseb_dev, 0, sizeof(float) * nb)); }
        if (nb && !c->topb_host) HIPCHK(c, hipHostMalloc((void**)&c->topb_host, sizeof(TopRec) * nb, hipHostMallocDefault));
        if (nb && !c->lseb_host) HIPCHK(c, hipHostMalloc((void**)&c->lseb_host, sizeof(float) * nb, hipHostMallocDefault));
        if (!c->top_scratch) HIPCHK(c, hipMalloc(&c->top_scratch, sizeof(TopRec) * (size_t)DTK_MAX_BATCH * DTK_TOP_MAX_SLICES));
      }
      c->top_logprobs = value; drop_graph(c); drop_batch_graphs(c);
    }
  }
  else if (!strcmp(name, "top_kernel") || !strcmp(name, "top_slice")) {     // which kernel leaves the records of "top_logprobs" (top_logits_launch); same bits
    const bool kern = !strcmp(name, "top_kernel");
    if (kern && (value < 0 || value > 2)) return fail(c, DTK_ERR_ARG, "top_kernel must be 0 (by vocabulary), 1 (k_top_logits) or 2 (k_top_slice + k_top_merge)");
    if (!kern && !top_sliced_ok(c->V, value))
      return fail(c, DTK_ERR_ARG, "top_slice must be 1 .. %d with at most %d slices of the vocabulary (%d)", DTK_TOP_MAX_L, DTK_TOP_MAX_SLICES, c->V);
    if (kern && value == 2 && !top_sliced_ok(c->V, c->top_slice))
      return fail(c, DTK_ERR_ARG, "top_kernel = 2: the vocabulary (%d) has more than %d slices of %d", c->V, DTK_TOP_MAX_SLICES, c->top_slice);
    if (value != (kern ? c->top_kernel : c->top_slice)) {
      if (c->blaunched != c->bwaited) return fail(c, DTK_ERR_STATE, "%s: a batch step is in flight", name);
      if (c->engine_holds.load() > 0) return fail(c, DTK_ERR_STATE, "%s: an engine holds %d sequence(s) in this context's slots", name, c->engine_holds.load());
      if (c->launched != c->waited) return fail(c, DTK_ERR_STATE, "%s: %d single-sequence decode step(s) are unread", name, (int)(c->launched - c->waited));
      (kern ? c->top_kernel : c->top_slice) = value; drop_graph(c); drop_batch_graphs(c);
    }
  }
  else if (!strcmp(name, "gemm_tile")) {   // MFMA GEMM block tile: 0 auto, 1 = 64x64, 2 = 128x64, 3 = 128x128 (process-wide)
    if (value < 0 || value > 5) return fail(c, DTK_ERR_ARG, "gemm_tile must be 0..5");
    set_gemm_tile(value);
  }
  else if (!strcmp(name, "share_prefix_reads")) c->share_reads = value != 0;
  else if (!strcmp(name, "prefix_mfma") || !strcmp(name, "pfx_splits") || !strcmp(name, "gemv_b_wide") ||
           !strcmp(name, "tail_threads")) {
    if (!strcmp(name, "prefix_mfma")) c->prefix_mfma = value != 0;
    else if (!strcmp(name, "tail_threads")) { if (value != 64 && value != 128 && value != 256 && value != 512) return fail(c, DTK_ERR_ARG, "tail_threads must be 64, 128, 256 or 512"); c->tail_threads = value; }
    else if (!strcmp(name, "pfx_splits")) { if (value < 1 || value > 4) return fail(c, DTK_ERR_ARG, "pfx_splits must be 1..4"); c->pfx_splits = value; }
    else { if (value < 0 || value > 6) return fail(c, DTK_ERR_ARG, "gemv_b_wide must be 0..6"); set_gemv_b_wide(value); }
    drop_batch_graphs(c);
  }
  else if (!strcmp(name, "gemm_impl")) {
    if (value < 0 || value > 4 || value == 1) return fail(c, DTK_ERR_ARG, "gemm_impl must be 0 (registers), 2 (k_gemm_glds where the shape has the tiles), 3 (auto) or 4 (k_gemm_g3: 8 waves, 3 LDS stages)");
    set_gemm_impl(value);
  }
  else if (!strcmp(name, "gemm_g3_min_blocks")) {
    if (value < 1) return fail(c, DTK_ERR_ARG, "gemm_g3_min_blocks must be >= 1");
    set_gemm_g3_min_blocks(value);
  }
  else if (!strcmp(name, "gemm_g3_tile")) {   // block tile of the one-chain k_gemm_g3: 0 = by shape, 1 = 256 x 128, 2 = 128 x 256 (process-wide; bit-identical)
    if (value < 0 || value > 2) return fail(c, DTK_ERR_ARG, "gemm_g3_tile must be 0, 1 or 2");
    set_gemm_g3_tile(value);
  }
  else if (!strcmp(name, "gemm_glds_min_tiles")) {
    if (value < 1) return fail(c, DTK_ERR_ARG, "gemm_glds_min_tiles must be >= 1");
    set_gemm_glds_min_tiles(value);
  }
  else if (!strcmp(name, "gqa_fused")) {
    if (value < 0 || value > 2) return fail(c, DTK_ERR_ARG, "gqa_fused must be 0 (a block per query head), 1 (per K/V head) or 2 (per pair of query heads)");
    c->gqa_fused = value;
    drop_batch_graphs(c);
  }
  else if (!strcmp(name, "resid_split")) {
    set_resid_split(value != 0);
    drop_batch_graphs(c);
  }
  else if (!strcmp(name, "gemv_bkl")) { set_gemv_bkl(value != 0); drop_batch_graphs(c); }
  else if (!strcmp(name, "gemv_bus")) { set_gemv_bus(value); drop_batch_graphs(c); }          // 64-slot qkv / gate-up by k_gemv_bus (kernels_batch_ks.hip): 0 off, 128 default per role, bit 0 qkv, bit 1 gate/up
  else if (!strcmp(name, "act_fp8")) {          // fp8 models: the MFMA-family step on the fp8 matrix cores with MXFP8 activations (kernels_batch_mx.hip)
    if (value && c->wfmt == 1 && c->nb > 0 && !c->mx_ok) return fail(c, DTK_ERR_ARG, "act_fp8: the model's shapes are not covered by the fp8 matrix-core kernels");
    c->act_fp8 = value != 0;
    drop_batch_graphs(c);
  }
  else if (!strcmp(name, "mx_nc_qkv") || !strcmp(name, "mx_nc_gu") || !strcmp(name, "mx_nc_lm_head")) {   // compute waves per block of k_gemv_mxu (0 = from the CU count)
    if (value < 0 || value > 4) return fail(c, DTK_ERR_ARG, "%s must be 0..4", name);
    set_mx_nc(!strcmp(name, "mx_nc_qkv") ? 0 : (!strcmp(name, "mx_nc_gu") ? 1 : 2), value);
    drop_batch_graphs(c);
  }
  else if (!strcmp(name, "gemv_br_wd")) { if (value != 4 && value != 8) return fail(c, DTK_ERR_ARG, "gemv_br_wd must be 4 or 8"); set_gemv_br_wd(value); drop_batch_graphs(c); }
  else if (!strcmp(name, "gemv_loaders")) { set_gemv_loaders(value >= 2 ? 2 : 1); drop_batch_graphs(c); }
  else if (!strcmp(name, "gemv_xw")) { set_gemv_xw(value < 0 ? 0 : (value > 2 ? 2 : value)); drop_batch_graphs(c); }   // x waves of k_gemv_bl / k_gemv_bkl
  else if (!strcmp(name, "gemv_bc")) {
    if (value < 0 || value > 255) return fail(c, DTK_ERR_ARG, "gemv_bc must be 0..255 (0 off; 128 = the measured default per role and weight format; else bit 0 qkv, bit 1 gate/up, bit 2 lm_head through k_gemv_bc; bits 4..6 = units per block, 0 = one CU's share)");
    set_gemv_bc(value);
    drop_batch_graphs(c);
  }
  else if (!strcmp(name, "gemv_bl")) {
    if (value < 0 || value > 127) return fail(c, DTK_ERR_ARG, "gemv_bl must be 0..127 (bit 6: bf16 qkv through k_gemv_br; bit 0: gate/up + lm_head, bit 1: qkv by pair units, bit 2: fp8 weights too, bit 3: qkv as pair + V tile per block where that fills the chip, bit 4: for any MHA model, bit 5: fp8 weights through registers (k_gemv_br, K = 4096))");
    set_gemv_bl(value);
    drop_batch_graphs(c);
  }
  else if (!strcmp(name, "attn_nt")) { c->attn_nt = value != 0; drop_batch_graphs(c); }
  else if (!strcmp(name, "mv_slots")) {     // contexts with at most value + 1 slots decode with the multi-vector kernels (0 = never)
    if (value < 0 || value > 4) return fail(c, DTK_ERR_ARG, "mv_slots must be 0..4");
    if (c->blaunched != c->bwaited) return fail(c, DTK_ERR_STATE, "mv_slots: a batch step is in flight");
    c->mv_slots = value;
    drop_batch_graphs(c);
  }
  else if (!strcmp(name, "mv_tail_threads")) {
    if (value != 256 && value != 512 && value != 1024) return fail(c, DTK_ERR_ARG, "mv_tail_threads must be 256, 512 or 1024");
    // GQA models run the group-fused blocks of k_attn_tail_b, which exist for fewer block sizes (launch_attn_decode_b): a value without
    // an instantiation used to be accepted and silently ignored
    const int grp = c->KVH > 0 ? c->H / c->KVH : 1;
    if (grp == 4 && value == 1024) return fail(c, DTK_ERR_ARG, "mv_tail_threads: GQA groups of 4 have blocks of 256 or 512 threads");
    if (grp == 2 && value != 256) return fail(c, DTK_ERR_ARG, "mv_tail_threads: GQA groups of 2 have blocks of 256 threads only");
    c->mv_tail_threads = value;
    drop_batch_graphs(c);
  }
  else if (!strncmp(name, "mv_shape_", 9)) {   // block shape of one multi-vector role: qkv | o | gu | down | lm_head; 0..3, -1 = measured default
    const char* r = name + 9;
    const int role = !strcmp(r, "qkv") ? EPI_QKV : !strcmp(r, "o") ? 5 : !strcmp(r, "gu") ? EPI_SWIGLU : !strcmp(r, "down") ? EPI_RESID : !strcmp(r, "lm_head") ? EPI_LOGITS : -1;
    if (role < 0 || value < -1 || value > 3) return fail(c, DTK_ERR_ARG, "mv_shape_{qkv,o,gu,down,lm_head} must be -1..3");
    set_gemv_mv_shape(role, value);
    drop_batch_graphs(c);
  }
  else if (!strcmp(name, "resid_kparts")) {     // batched N = d roles as k_gemv_bkp + k_resid_norm_b (64 slots, bf16 weights)
    c->resid_kparts = value != 0;
    drop_batch_graphs(c);
  }
  else if (!strcmp(name, "gemv_bx")) {
    if (value < 0 || value > 4) return fail(c, DTK_ERR_ARG, "gemv_bx must be 0..4");
    set_gemv_bx(value);
    drop_batch_graphs(c);
  }
  else if (!strcmp(name, "gemm_ring")) {
    if (value < 2 || value > 4) return fail(c, DTK_ERR_ARG, "gemm_ring must be 2..4");
    set_gemm_ring(value);
  }
  else if (!strcmp(name, "vit_feature_layer")) {   // diagnostic (per-block parity tests): which block's normed output dtk_vit_encode(feats) returns
    if (value < 0 || value >= c->vDepth) return fail(c, DTK_ERR_ARG, "vit_feature_layer must be 0..%d", c->vDepth - 1);
    HIPCHK(c, hipStreamSynchronize(c->stream_vit));
    c->cfg.vit_feature_layer = value;
    c->have_image = false; c->cached_image_key = 0;   // a cached image prefix was projected from the old layer's features
    c->seq0.image_key = 0; c->seq0.cached_ids.clear();
    for (SeqHost& sh : c->bseq) { sh.image_key = 0; sh.cached_ids.clear(); sh.share_src = -1; sh.share_len = 0; }
    pen_clear_all(c);
  }
  else if (!strcmp(name, "qkv_rope_fused")) c->qkv_rope_fused = value != 0;
  else if (!strcmp(name, "swiglu_fused")) c->swiglu_fused = value != 0;
  else if (!strcmp(name, "sk_sl_min_rows")) { if (value < 1) return fail(c, DTK_ERR_ARG, "sk_sl_min_rows must be >= 1"); c->sk_sl_min_rows = value; }
  else if (!strcmp(name, "gemm_epi_direct")) set_gemm_epi_direct(value != 0);   // k_gemm_g3 without the LDS-transposed epilogue (default 0; process-wide; bit-identical)
  else if (!strcmp(name, "gemm_wt")) set_gemm_wt(value != 0);     // k_gemm_g3's W stage from the fragment-major copy (default 1; process-wide; bit-identical)
  else if (!strcmp(name, "gemm_sk_tile")) {   // block tile of the sliced-K GEMM: 0 = 256 x 128, 1 = 128 x 256, 2 = by M (process-wide; bit-identical)
    if (value < 0 || value > 2) return fail(c, DTK_ERR_ARG, "gemm_sk_tile must be 0, 1 or 2");
    set_gemm_sk_tile(value);
  }
  else if (!strcmp(name, "prefill_sk")) {   // sliced-K prefill GEMMs (default 1).  The two settings round differently: cached prefixes are dropped
    if (value < 0 || value > 8 || (value & (value - 1))) return fail(c, DTK_ERR_ARG, "prefill_sk must be 0 (one-chain GEMMs), 1 (sliced by the weight shape: the default) or a cap of 2 / 4 / 8 slices");
    c->prefill_sk = value;
    c->seq0.cached_ids.clear();
    for (SeqHost& sh : c->bseq) { sh.cached_ids.clear(); sh.share_src = -1; sh.share_len = 0; }
    pen_clear_all(c);
  }
  else if (!strcmp(name, "gemm_bk")) {
    if (value != 64 && value != 128) return fail(c, DTK_ERR_ARG, "gemm_bk must be 64 or 128");
    set_gemm_bk(value);
  }
  else if (!strcmp(name, "gemm_stages")) {
    if (value < 1 || value > 4) return fail(c, DTK_ERR_ARG, "gemm_stages must be 1..4");
    set_gemm_stages(value);
  }
  else if (!strcmp(name, "attn_impl")) {   // prefill / ViT attention: 0 auto, 1 VALU kernel, 2 MFMA flash kernel
    if (value < 0 || value > 2) return fail(c, DTK_ERR_ARG, "attn_impl must be 0..2");
    c->attn_impl = value;
  }
  else if (!strcmp(name, "attn_threads") || !strcmp(name, "attn_splits") || !strcmp(name, "attn_combine")) {
    if (!strcmp(name, "attn_threads")) {
      if (value != 0 && value != 256 && value != 512 && value != 1024) return fail(c, DTK_ERR_ARG, "attn_threads must be 0, 256, 512 or 1024");
      if (value == 0 && c->hd == 64) return fail(c, DTK_ERR_ARG, "attn_threads 0 (contiguous splits) has no head_dim-64 kernel: 256, 512 or 1024");
      c->attn_threads = value;
    } else if (!strcmp(name, "attn_splits")) {
      if (value < 1 || value > 16) return fail(c, DTK_ERR_ARG, "attn_splits must be 1..16");
      c->S = value;
    } else {
      if (value < 0 || value > 2) return fail(c, DTK_ERR_ARG, "attn_combine must be 0..2");
      c->attn_combine = value;
    }
    drop_graph(c);
  } else return fail(c, DTK_ERR_ARG, "unknown option '%s'", name);
  return DTK_OK;
}

int dtk_set_gemv_variant(dtk_ctx* c, int epi, int variant) {
  if (!c) return DTK_ERR_ARG;
  drop_graph(c);
  set_gemv_default_variant(epi, variant);
  return DTK_OK;
}

// ---- TikZero adapter (ABI 7) ------------------------------------------------------------------------------------------------------
static void plan_adapter(dtk_ctx* c, Adapter& A, Planner& P, bool reg) {
  const int D = c->vD, mlp = c->vMlp, hd = c->vHd, de = A.cfg.hidden, Tt = A.cfg.text_max;
  const size_t img = (size_t)3 * c->cfg.vit_image * c->cfg.vit_image;
  const float ws = 0.02f;
  auto R = [&](const std::string& n, bf16_t* p, int64_t r, int64_t cl, float sc, float of) { if (reg) add_tensor(c, n, p, r, cl, cl, sc, of); };
  A.conn_w = P.take<bf16_t>((size_t)D * de); A.conn_b = P.take<bf16_t>(D);
  R("adapter.connector.weight", A.conn_w, D, de, ws, 0.f);
  R("adapter.connector.bias", A.conn_b, 1, D, 0.01f, 0.f);
  A.dummy = P.take<bf16_t>(img);
  R("adapter.dummy_input", A.dummy, 1, (int64_t)img, 1.5f, 0.f);      // synthetic: partly outside [-1, 1], so the clamp is exercised
  A.ctext = P.take<bf16_t>((size_t)Tt * D);
  if (reg) { A.layers.assign((size_t)c->vDepth, CrossW{}); A.present.assign((size_t)c->vDepth, 0); }
  for (int i = 0; i < c->vDepth; ++i) {
    if ((i + 1) % A.cfg.every_n != 0) continue;
    CrossW w{};
    w.ln1w = P.take<bf16_t>(D); w.ln1b = P.take<bf16_t>(D);
    w.qw = P.take<bf16_t>((size_t)D * D); w.qb = P.take<bf16_t>(D);
    w.kw = P.take<bf16_t>((size_t)D * D); w.kb = P.take<bf16_t>(D);
    w.vw = P.take<bf16_t>((size_t)D * D); w.vb = P.take<bf16_t>(D);
    w.ow = P.take<bf16_t>((size_t)D * D); w.ob = P.take<bf16_t>(D);
    w.qnw = P.take<bf16_t>(hd); w.qnb = P.take<bf16_t>(hd); w.knw = P.take<bf16_t>(hd); w.knb = P.take<bf16_t>(hd);
    w.ln2w = P.take<bf16_t>(D); w.ln2b = P.take<bf16_t>(D);
    w.f1w = P.take<bf16_t>((size_t)mlp * D); w.f1b = P.take<bf16_t>(mlp);
    w.f2w = P.take<bf16_t>((size_t)D * mlp); w.f2b = P.take<bf16_t>(D);
    w.gate_a = P.take<bf16_t>(1); w.gate_m = P.take<bf16_t>(1);
    w.K = P.take<bf16_t>((size_t)Tt * D); w.V = P.take<bf16_t>((size_t)Tt * D);
    if (!reg) continue;
    A.layers[(size_t)i] = w; A.present[(size_t)i] = 1;
    const std::string p = "adapter.layers." + std::to_string(i) + ".";
    R(p + "layer_norm1.weight", w.ln1w, 1, D, 0.1f, 1.f); R(p + "layer_norm1.bias", w.ln1b, 1, D, 0.01f, 0.f);
    R(p + "cross_attn.q_proj.weight", w.qw, D, D, ws, 0.f); R(p + "cross_attn.q_proj.bias", w.qb, 1, D, 0.01f, 0.f);
    R(p + "cross_attn.k_proj.weight", w.kw, D, D, ws, 0.f); R(p + "cross_attn.k_proj.bias", w.kb, 1, D, 0.01f, 0.f);
    R(p + "cross_attn.v_proj.weight", w.vw, D, D, ws, 0.f); R(p + "cross_attn.v_proj.bias", w.vb, 1, D, 0.01f, 0.f);
    R(p + "cross_attn.out_proj.weight", w.ow, D, D, ws, 0.f); R(p + "cross_attn.out_proj.bias", w.ob, 1, D, 0.01f, 0.f);
    R(p + "cross_attn.q_norm.weight", w.qnw, 1, hd, 0.1f, 1.f); R(p + "cross_attn.q_norm.bias", w.qnb, 1, hd, 0.01f, 0.f);
    R(p + "cross_attn.k_norm.weight", w.knw, 1, hd, 0.1f, 1.f); R(p + "cross_attn.k_norm.bias", w.knb, 1, hd, 0.01f, 0.f);
    R(p + "layer_norm2.weight", w.ln2w, 1, D, 0.1f, 1.f); R(p + "layer_norm2.bias", w.ln2b, 1, D, 0.01f, 0.f);
    R(p + "mlp.fc1.weight", w.f1w, mlp, D, ws, 0.f); R(p + "mlp.fc1.bias", w.f1b, 1, mlp, 0.01f, 0.f);
    R(p + "mlp.fc2.weight", w.f2w, D, mlp, ws, 0.f); R(p + "mlp.fc2.bias", w.f2b, 1, D, 0.01f, 0.f);
    // gates: a trained adapter's are far from 0; synthetic ones are too (at 0 every gate would be 0.5 and nothing would show it is read)
    R(p + "cross_attn_attn_gate", w.gate_a, 1, 1, 1.0f, 0.5f); R(p + "cross_attn_mlp_gate", w.gate_m, 1, 1, 1.0f, -0.5f);
  }
}

int dtk_adapter_create(dtk_ctx* c, const dtk_adapter_config* cfg) {
  if (!c || !cfg) return fail(c, DTK_ERR_ARG, "dtk_adapter_create: null argument");
  if (c->ad) return fail(c, DTK_ERR_STATE, "an adapter is loaded already (dtk_adapter_destroy first)");
  // the reference's hooks look for the HF SigLIP ModuleList; a v1 checkpoint's timm tower has none (add_hooks raises)
  if (c->proj_bias) return fail(c, DTK_ERR_ARG, "Couldn't locate vision encoder layers! (the TikZero adapter needs a v2 checkpoint's SigLIP tower)");
  if (cfg->every_n < 1 || cfg->text_max < 1 || cfg->text_max > 4096)
    return fail(c, DTK_ERR_ARG, "adapter: every_n %d / text_max %d out of range", cfg->every_n, cfg->text_max);
  HIPCHK(c, hipSetDevice(c->device));
  std::lock_guard<std::mutex> vit_guard(c->vit_mu);
  dtk_config ec{};
  ec.hidden = cfg->hidden; ec.layers = cfg->layers; ec.heads = cfg->heads; ec.head_dim = cfg->head_dim; ec.ffn = cfg->ffn;
  ec.vocab = cfg->vocab; ec.max_positions = cfg->text_max < 8 ? 8 : cfg->text_max; ec.rms_eps = cfg->rms_eps;
  ec.rope_theta = cfg->rope_theta; ec.rope_factor = cfg->rope_factor;
  // the embedding model has no tower: the smallest one dtk_create accepts (one 14 px patch), allocated, never run
  ec.vit_dim = 32; ec.vit_depth = 1; ec.vit_heads = 1; ec.vit_mlp = 32; ec.vit_patch = 14; ec.vit_image = 14;
  ec.vit_feature_layer = 0; ec.vit_ln_eps = 1e-6f; ec.concat_patches = 1; ec.image_token_id = -1;
  ec.reserved[2] = cfg->kv_heads == cfg->heads ? 0 : cfg->kv_heads;
  ec.reserved[3] = DTK_ARCH_PROJ_NO_BIAS;
  Adapter* A = new Adapter();
  A->cfg = *cfg;
  if (dtk_create(&ec, c->device, &A->emb) != DTK_OK) {
    const std::string why = g_create_error;
    delete A;
    return fail(c, DTK_ERR_ARG, "adapter embedding model: %s", why.c_str());
  }
  Planner sz;
  plan_adapter(c, *A, sz, false);
  const size_t bytes = align_up(sz.off, 256) + 256;
  if (hipMalloc((void**)&A->arena, bytes) != hipSuccess) { dtk_destroy(A->emb); delete A; return fail(c, DTK_ERR_HIP, "adapter: hipMalloc of %zu bytes failed", bytes); }
  (void)hipMemsetAsync(A->arena, 0, bytes, c->stream);
  (void)hipStreamSynchronize(c->stream);
  A->first_tensor = c->tensors.size();
  Planner real;
  real.base = A->arena;
  plan_adapter(c, *A, real, true);
  // the embedding model's tensors under the reference's names (AutoModel's state dict: no "model." prefix, no head)
  for (const TensorEntry& t : A->emb->tensors) {
    std::string n = t.name;
    if (n.compare(0, 6, "model.") == 0 && n.compare(0, 16, "model.mm_project") != 0) n = n.substr(6);
    else if (n != "rope.cos" && n != "rope.sin") continue;
    add_tensor(c, "embedding_model." + n, t.ptr, t.rows, t.cols, t.stride, t.synth_scale, t.synth_offset);
  }
  c->ad = A;
  c->have_image = false;                 // nothing cached before the adapter was there is keyed by a text
  return DTK_OK;
}

int dtk_adapter_destroy(dtk_ctx* c) {
  if (!c) return DTK_ERR_ARG;
  if (!c->ad) return DTK_OK;
  (void)hipSetDevice(c->device);
  std::lock_guard<std::mutex> vit_guard(c->vit_mu);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->stream_vit) (void)hipStreamSynchronize(c->stream_vit);
  Adapter* A = c->ad;
  for (size_t i = A->first_tensor; i < c->tensors.size(); ++i) c->tindex.erase(c->tensors[i].name);
  c->tensors.resize(A->first_tensor);
  if (A->arena) (void)hipFree(A->arena);
  dtk_destroy(A->emb);
  delete A;
  c->ad = nullptr;
  c->have_image = false;                 // a text-conditioned image may be cached: drop every cached prefix
  c->seq0.cached_ids.clear();
  for (auto& b : c->bseq) b.cached_ids.clear();
  pen_clear_all(c);
  return DTK_OK;
}

int dtk_has_adapter(const dtk_ctx* c) { return (c && c->ad) ? 1 : 0; }

uint64_t dtk_text_image_key(uint64_t image_key, uint64_t text_key) {
  if (image_key == 0 || text_key == 0) return 0;
  uint64_t z = image_key ^ (text_key * 0x9E3779B97F4A7C15ull) ^ 0x5445585443524F53ull;    // splitmix64 finaliser of the pair
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z ? z : 1;
}

int dtk_vit_encode_text(dtk_ctx* c, const float* pixels, int batch, const int64_t* text_ids, int T_text, uint64_t text_key,
                        void* feats_out, void* pooled_out) {
  (void)text_key;      // the text cache compares the ids themselves
  if (!c || batch < 1 || !text_ids) return fail(c, DTK_ERR_ARG, "dtk_vit_encode_text: bad argument");
  if (!c->ad) return fail(c, DTK_ERR_STATE, "no adapter loaded (dtk_adapter_create)");
  std::vector<float> dummy;
  if (!pixels) {
    std::lock_guard<std::mutex> vit_guard(c->vit_mu);
    const int rc = dummy_pixels(c, batch, dummy);
    if (rc != DTK_OK) return rc;
    pixels = dummy.data();
  }
  return vit_encode_impl(c, pixels, batch, feats_out, pooled_out, text_ids, T_text);
}

static int prefill_text_common(dtk_ctx* c, const float*& pixels, std::vector<float>& dummy, const int64_t* text_ids) {
  if (!c) return DTK_ERR_ARG;
  if (!text_ids) return fail(c, DTK_ERR_ARG, "dtk_prefill_text: no text");
  if (!c->ad) return fail(c, DTK_ERR_STATE, "no adapter loaded (dtk_adapter_create)");
  if (!pixels) {
    std::lock_guard<std::mutex> vit_guard(c->vit_mu);
    const int rc = dummy_pixels(c, 1, dummy);
    if (rc != DTK_OK) return rc;
    pixels = dummy.data();
  }
  return DTK_OK;
}

int dtk_prefill_text(dtk_ctx* c, const int64_t* ids, int T, const float* pixels, uint64_t image_key,
                     const int64_t* text_ids, int T_text, uint64_t text_key, int flags, float* logits_out) {
  std::vector<float> dummy;
  const int rc = prefill_text_common(c, pixels, dummy, text_ids);
  if (rc != DTK_OK) return rc;
  return prefill_impl(c, c->seq0, c->kv, c->logits, c->st, true, ids, T, pixels, dtk_text_image_key(image_key, text_key), flags, logits_out,
                      text_ids, T_text);
}

int dtk_score_text(dtk_ctx* c, const int64_t* ids, int T, const float* pixels, uint64_t image_key, const int64_t* text_ids, int T_text,
                   uint64_t text_key, uint32_t flags, int first, float* logprob_out, int32_t* argmax_out, float* lse_out) {
  return dtk_score_top_text(c, ids, T, pixels, image_key, text_ids, T_text, text_key, flags, first, logprob_out, argmax_out, lse_out, 0, nullptr, nullptr);
}

int dtk_score_top_text(dtk_ctx* c, const int64_t* ids, int T, const float* pixels, uint64_t image_key, const int64_t* text_ids, int T_text,
                       uint64_t text_key, uint32_t flags, int first, float* logprob_out, int32_t* argmax_out, float* lse_out,
                       int k, int32_t* top_ids_out, float* top_logprob_out) {
  if (!c) return DTK_ERR_ARG;
  const int rc0 = score_check(c, ids, T, first, logprob_out, k, top_ids_out, top_logprob_out);
  if (rc0 != DTK_OK) return rc0;
  std::vector<float> dummy;
  const int rc = prefill_text_common(c, pixels, dummy, text_ids);
  if (rc != DTK_OK) return rc;
  const ScoreReq rq{first, logprob_out, argmax_out, lse_out, k, top_ids_out, top_logprob_out};
  return prefill_impl(c, c->seq0, c->kv, c->logits, c->st, true, ids, T, pixels, dtk_text_image_key(image_key, text_key), (int)flags, nullptr,
                      text_ids, T_text, &rq);
}

int dtk_score_packed_text(dtk_ctx* c, const int64_t* prefix_ids, int P, const float* pixels, uint64_t image_key, const int64_t* text_ids,
                          int T_text, uint64_t text_key, uint32_t flags, const int64_t* cand_ids, const int32_t* cand_len, int N,
                          float* logprob_out, int32_t* argmax_out, float* lse_out) {
  return dtk_score_packed_top_text(c, prefix_ids, P, pixels, image_key, text_ids, T_text, text_key, flags, cand_ids, cand_len, N, logprob_out,
                                   argmax_out, lse_out, 0, nullptr, nullptr);
}

int dtk_score_packed_top_text(dtk_ctx* c, const int64_t* prefix_ids, int P, const float* pixels, uint64_t image_key, const int64_t* text_ids,
                              int T_text, uint64_t text_key, uint32_t flags, const int64_t* cand_ids, const int32_t* cand_len, int N,
                              float* logprob_out, int32_t* argmax_out, float* lse_out, int k, int32_t* top_ids_out, float* top_logprob_out) {
  if (!c) return DTK_ERR_ARG;
  const PackedReq rq{prefix_ids, P, cand_ids, cand_len, N, logprob_out, argmax_out, lse_out, k, top_ids_out, top_logprob_out};
  int total = 0;
  const int rc0 = packed_check(c, rq, &total);
  if (rc0 != DTK_OK) return rc0;
  std::vector<float> dummy;
  const int rc = prefill_text_common(c, pixels, dummy, text_ids);
  if (rc != DTK_OK) return rc;
  return score_packed_impl(c, rq, total, pixels, dtk_text_image_key(image_key, text_key), (int)flags, text_ids, T_text);
}

int dtk_prefill_slot_text(dtk_ctx* c, int slot, const int64_t* ids, int T, const float* pixels, uint64_t image_key,
                          const int64_t* text_ids, int T_text, uint64_t text_key, int flags, float* logits_out) {
  if (!c || slot < 0 || slot >= c->nb) return fail(c, DTK_ERR_ARG, "dtk_prefill_slot_text: slot %d of %d", slot, c ? c->nb : 0);
  std::vector<float> dummy;
  const int rc0 = prefill_text_common(c, pixels, dummy, text_ids);
  if (rc0 != DTK_OK) return rc0;
  SeqHost& sh = c->bseq[(size_t)slot];
  sh.last_reuse_start = 0;
  const int rc = prefill_impl(c, sh, c->kvb + (size_t)slot * c->kv_slot_stride, c->logits_b + (size_t)slot * c->V,
                              c->st_b + slot, false, ids, T, pixels, dtk_text_image_key(image_key, text_key), flags, logits_out,
                              text_ids, T_text);
  const int kept = rc == DTK_OK ? sh.last_reuse_start : 0;       // as dtk_prefill_slot
  auto clip = [&](SeqHost& q) { q.share_len = std::min(q.share_len, kept); if (q.share_len <= 0) { q.share_src = -1; q.share_len = 0; } };
  clip(sh);
  for (int j = 0; j < c->nb; ++j)
    if (j != slot && c->bseq[(size_t)j].share_src == slot) clip(c->bseq[(size_t)j]);
  if (rc == DTK_OK) sh.kv8_from = sh.host_next_pos;      // every row of the slot is now a prefill row (kept ones included): bf16 only
  else sh.kv8_from = std::min(sh.kv8_from, sh.host_next_pos);      // a refused or failed prefill may have cut the context: never above its length
  return rc;
}

int dtk_adapter_embed(dtk_ctx* c, const int64_t* text_ids, int T_text, void* hidden_out) {
  if (!c || !text_ids || !hidden_out) return fail(c, DTK_ERR_ARG, "dtk_adapter_embed: bad argument");
  if (!c->ad) return fail(c, DTK_ERR_STATE, "no adapter loaded (dtk_adapter_create)");
  std::lock_guard<std::mutex> vit_guard(c->vit_mu);
  dtk_ctx* e = c->ad->emb;
  if (embed_pass(e, text_ids, T_text) != DTK_OK) return fail(c, DTK_ERR_STATE, "adapter embedding pass: %s", e->err.c_str());
  HIPCHK(c, hipMemcpy(hidden_out, e->Xn, (size_t)T_text * e->d * 2, hipMemcpyDeviceToHost));
  return DTK_OK;
}


}  // extern "C"
#pragma GCC visibility pop
