// dtk_ctx.h — what the library's two host translation units share: the context (dtk_api.hip owns it and defines everything declared
// here) and the product helpers the op-level test entry points (dtk_ops.hip) call.  Internal: not installed, nothing in it is exported
// (the library is built with -fvisibility=hidden and this header is included outside any visibility pragma).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/dtk.h"
#include "kernels.h"
#ifndef W13_DEFAULT
#define W13_DEFAULT 1      // option "w13" of a new context (on: DESIGN 3.1c'')
#endif

struct TensorEntry {
  std::string name;
  bf16_t* ptr = nullptr;   // destination (view into the arena)
  int64_t rows = 1;        // logical rows
  int64_t cols = 0;        // logical row length (elements)
  int64_t stride = 0;      // destination row stride (elements), >= cols
  float synth_scale = 0.02f;
  float synth_offset = 0.f;
  bool loaded = false;     // written by dtk_load_tensor / dtk_fill_synthetic
  int64_t numel() const { return rows * cols; }
};

struct SeqHost {   // host-side mirror of one sequence's decode state
  std::vector<int64_t> cached_ids;
  bool cached_with_image = false;  // the cached KV was computed with image features spliced in
  uint64_t image_key = 0;          // ... of the image with this caller-supplied key (0 = unknown: never reused across images)
  int host_next_pos = 0;           // tokens with KV after all launched steps
  bool have_logits = false;
  int share_src = -1;              // slot whose first share_len cached tokens are bit-identical to ours (dtk_kv_fork), or -1
  int share_len = 0;
  int last_reuse_start = 0;        // tokens of the previous cache the last prefill kept
  int64_t forced_pending = -1;     // dtk_resume_slot's last id until the step that forwards it is launched: part of the sequence, not yet of cached_ids
  int kv8_from = 0;                // kv_format "mxfp8": rows [kv8_from, length) were written by decode steps and have MXFP8 shadow rows (BatchState::kv8_from)
};

struct LayerW {
  bf16_t *wqkv, *wo, *wgu, *wdown, *ln1, *ln2;
  bf16_t *t_wqkv = nullptr, *t_wo = nullptr, *t_wgu = nullptr, *t_wdown = nullptr;  // fragment-major copies (batched decode)
  bf16_t *p_wqkv = nullptr, *p_wo = nullptr, *p_wgu = nullptr, *p_wdown = nullptr;  // fragment-major bf16 copies the prefill GEMMs stream (= t_* where those exist)
  bf16_t* p_wgui = nullptr;          // gate/up again with its row tiles in (gate, up) pair order: the W stage of the SwiGLU-fused prefill GEMM (models whose gate/up role is one chain)
  uint8_t *q_wqkv = nullptr, *q_wo = nullptr, *q_wgu = nullptr, *q_wdown = nullptr;  // fp8 e4m3 copies (weight_format 1)
  float *s_wqkv = nullptr, *s_wo = nullptr, *s_wgu = nullptr, *s_wdown = nullptr;    // per-row power-of-two scales
  uint8_t *f4_wqkv = nullptr, *f4_wo = nullptr, *f4_wgu = nullptr, *f4_wdown = nullptr;  // MXFP4 E2M1 codes (weight_format 2): [N][ceil(K/32)*16] bytes
  uint8_t *e4_wqkv = nullptr, *e4_wo = nullptr, *e4_wgu = nullptr, *e4_wdown = nullptr;  // ... and their E8M0 block scales: [N][ceil(K/32)]
  uint8_t *p13_wqkv = nullptr, *p13_wo = nullptr, *p13_wgu = nullptr, *p13_wdown = nullptr;  // 13-bit planes of the bf16 rows (w13.h; bf16 contexts, option "w13"): null = not packed
  uint8_t *h13_wqkv = nullptr, *h13_wo = nullptr, *h13_wgu = nullptr, *h13_wdown = nullptr;  // ... and the rows' hb bytes
  uint8_t *t8_wqkv = nullptr, *t8_wo = nullptr, *t8_wgu = nullptr, *t8_wdown = nullptr;  // fp8 pair-tiled copies (batched decode, fp8)
  uint8_t *m_wqkv = nullptr, *m_wo = nullptr, *m_wgu = nullptr, *m_wdown = nullptr;      // fp8 MX tiles (fp8 matrix-core step; down in groups of 16)
};
struct VitBlockW {
  bf16_t *n1w, *n1b, *qkvw, *qkvb, *projw, *projb, *n2w, *n2b, *fc1w, *fc1b, *fc2w, *fc2b;
};
// one CrossAttentionLayer of the TikZero adapter (reference adapter/modeling_adapter.py) + the text's keys / values it attends to
struct CrossW {
  bf16_t *ln1w, *ln1b, *qw, *qb, *kw, *kb, *vw, *vb, *ow, *ob, *qnw, *qnb, *knw, *knb, *ln2w, *ln2b, *f1w, *f1b, *f2w, *f2b;
  bf16_t *gate_a, *gate_m;           // cross_attn_attn_gate / cross_attn_mlp_gate: one bf16 logit each
  bf16_t *K, *V;                     // the cached text's k_norm(k_proj(c)) / v_proj(c): [text_max][D]
};
struct Adapter {
  dtk_adapter_config cfg{};
  dtk_ctx* emb = nullptr;            // the embedding model: a decoder-only context (its tower is a 1-patch stub that never runs)
  unsigned char* arena = nullptr;
  size_t first_tensor = 0;           // the adapter's entries are the tail of the owner's tensor table from here on
  bf16_t *conn_w = nullptr, *conn_b = nullptr, *dummy = nullptr, *ctext = nullptr;
  std::vector<CrossW> layers;        // per ViT block; present[i]: a cross layer runs before block i
  std::vector<char> present;
  std::vector<int64_t> text_ids;     // the text whose connector output and k / v are cached (empty: none)
  std::vector<float> dummy_host;     // dummy_input.clamp(-1, 1) as fp32 pixels (empty: not built since the last weight load)
};

struct dtk_ctx {
  dtk_config cfg;
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  std::mutex err_mu;
  // dtk_vit_encode (own stream, any thread: the SelfSim rewards) and a prefill (the engine's loop thread) share the ViT activation
  // buffers and `cur_stream`: one at a time
  std::mutex vit_mu;

  // derived sizes
  int d, L, H, ff, V, Tmax, S;           // S: split-K factor of the single-sequence decode attention
  int vD, vDepth, vH, vHd, vMlp, vN, vPatchK, vPatchLd, nImg;

  // weights
  unsigned char* arena = nullptr;
  size_t arena_bytes = 0;
  std::vector<TensorEntry> tensors;
  std::unordered_map<std::string, int> tindex;
  std::vector<LayerW> layers;
  bf16_t *embed, *final_norm, *lm_head, *mm_w, *mm_b;
  bf16_t *rope_cos, *rope_sin;
  std::vector<VitBlockW> vblocks;
  bf16_t *pe_w, *pe_b, *pos_embed, *vnorm_w, *vnorm_b;
  bf16_t *ap_latent, *ap_qw, *ap_qb, *ap_kvw, *ap_kvb, *ap_pw, *ap_pb, *ap_nw, *ap_nb, *ap_f1w,
      *ap_f1b, *ap_f2w, *ap_f2b;

  // KV cache [L][2][KVH][Tmax][hd]
  bf16_t* kv = nullptr;

  // activations: decoder prefill
  bf16_t *X, *Xn, *QKV, *Qh, *AO, *GU, *ACT;
  int sk_sl_min_rows = SK_SL_MIN_ROWS;   // above this many rows a sliced role is one launch with the slices folded in registers (dtk_set_option "sk_sl_min_rows"; bit-identical)
  float* skpart = nullptr;           // fp32 partials of the sliced-K prefill GEMMs: [kslices][SK_CHUNK_ROWS][N], one role at a time
  size_t skpart_floats = 0;
  int swiglu_fused = 1;              // gate/up's epilogue is SiLU*mul (dtk_set_option "swiglu_fused"; bit-identical)
  int qkv_rope_fused = 1;            // a sliced q/k/v role reduces inside the RoPE + KV-append kernel (dtk_set_option "qkv_rope_fused"; bit-identical)
  int prefill_sk = 1;                // sliced-K prefill GEMMs for the roles with <= 128 tiles of 256 x 128 (dtk_set_option "prefill_sk": 0 = the one-chain kernels, 2 / 4 / 8 = a cap on the slices)
  int32_t* ids_dev = nullptr;
  // dtk_score / dtk_score_packed: records of the log-softmax lm_head ([max_positions][ceil(V / 128)] x 16 B: a packed pass behind a one-token prompt scores max_positions rows) + the per-row results; allocated by the first
  // scoring call and kept (hipMalloc of its own, not the arena: a context that never scores pays nothing)
  float* score_rec = nullptr;
  float* score_out = nullptr;         // [4][max_positions]: logprob, lse, argmax (int32), z[argmax]
  float* score_top = nullptr;         // dtk_score_top: [2][max_positions][DTK_MAX_TOP]: ids (int32), logprob; allocated by the first call with k > 0
  // dtk_score_packed: the row tables of one packed pass, [6][max_positions] int32 — {position, cache row} and {segment begin, cache row}
  // per row (int2 each), the rows' input ids, the scored rows' targets; allocated by the first packed call and kept
  int32_t* packed_rows = nullptr;
  // decode step
  bf16_t *x, *q, *act;
  float *logits, *pm, *pl, *po;
  bf16_t* attn_out = nullptr;        // combined attention output [d] (in-kernel combine)
  unsigned* attn_ctr = nullptr;      // [H] arrival tickets
  int attn_combine = 0;              // 0: consumer (o_proj prologue), 1: last-arriver in k_attn_decode, 2: own kernel
  DecState* st = nullptr;
  SamplingDev* sp = nullptr;
  int64_t* tok_ring_dev = nullptr;   // device ring
  int64_t* tok_ring_host = nullptr;  // pinned host mirror
  float* probs_dev = nullptr;        // op_sample output
  // dtk_set_option "logprobs": (logprob, sample_logprob) of every sampled token, rings parallel to tok_ring_* / tokb_* (same index)
  int logprobs = 0;
  std::atomic<int> engine_holds{0};  // sequences an engine of dtk_engine_create holds in this context's slots (joined, not yet left)
  float2* lp_ring_dev = nullptr;     // [DTK_MAX_INFLIGHT]
  float2* lp_ring_host = nullptr;    // pinned mirror
  float2* lpb_dev = nullptr;         // [DTK_MAX_INFLIGHT][DTK_MAX_BATCH] (contexts with slots)
  float2* lpb_host = nullptr;
  // dtk_set_option "top_logprobs" = k (needs "logprobs"): every step also leaves the k most likely tokens of the logits it sampled from
  // (k_top_logits, in front of the sampler) and the logsumexp its logprob was taken against; rings indexed as lp_ring / lpb.  Allocated
  // (hipMalloc / pinned, not the arena) when the option is first switched on
  int top_logprobs = 0;
  TopRec* top_ring_dev = nullptr;    // [DTK_MAX_INFLIGHT]
  TopRec* top_ring_host = nullptr;
  float* lse_ring_dev = nullptr;     // [DTK_MAX_INFLIGHT]
  float* lse_ring_host = nullptr;
  TopRec* topb_dev = nullptr;        // [DTK_MAX_INFLIGHT][DTK_MAX_BATCH] (contexts with slots)
  TopRec* topb_host = nullptr;
  float* lseb_dev = nullptr;
  float* lseb_host = nullptr;
  // which kernel leaves the records (top_logits_launch): "top_kernel" 0 = by vocabulary (the sliced pair where V > 8192: more than one slice), 1 =
  // k_top_logits, 2 = the sliced pair; "top_slice" = its L (tests run several slices at a small vocabulary with it)
  int top_kernel = 0;
  int top_slice = DTK_TOP_MAX_L;
  TopRec* top_scratch = nullptr;     // [DTK_MAX_BATCH][DTK_TOP_MAX_SLICES] the slices' candidates (allocated with the rings)
  // ViT
  float* pixels_dev = nullptr;
  bf16_t *patches, *VX, *VN, *VQKV, *VAO, *VH, *feats, *last_hidden;
  bf16_t *pq, *pkv, *pao, *px, *pn, *ph, *pooled;
  bf16_t* IMG;  // projected image embeddings [nImg][d]
  Adapter* ad = nullptr;             // TikZero text adapter (dtk_adapter_create), or none
  // op-level scratch
  unsigned char* scratch = nullptr;
  size_t scratch_bytes = 0;

  // host state
  SeqHost seq0;              // the single-sequence API (dtk_prefill / dtk_decode*)
  int wfmt = 0;              // 0 = bf16 decoder weights, 1 = fp8 e4m3 + per-row 2^e scale, 2 = MXFP4 layers + fp8 lm_head (dtk_config.reserved[1])
  bool fp8_ready = false;    // the quantised copies of wfmt 1 / 2 match the bf16 masters
  uint8_t* q_lm_head = nullptr;
  float* s_lm_head = nullptr;
  // 13-bit planes of the bf16 rows for the single-sequence step (w13.h): packed lazily by ensure_w13 from the bf16 masters, which stay
  int w13 = W13_DEFAULT;     // dtk_set_option "w13"
  int w13_nz = 1;            // dtk_set_option "w13_nz": 0 = the packer flags every row (W13_ZROW), so every row takes the general decode
  bool w13_ready = false;    // the planes match the masters (load_tensor / fill_synthetic clear it)
  uint8_t *p13_lm_head = nullptr, *h13_lm_head = nullptr;
  unsigned* w13_bad = nullptr;                      // device counter of the packer
  int w13_op_bad_rows = -1;                         // unpackable rows of the last dtk_op_gemv_role call that packed planes (-1: none yet)
  uint32_t w13_packed = 0, w13_unpacked = 0, w13_bad_rows = 0;   // matrices with / without planes, unpackable rows (dtk_stats.w13_counts)
  uint32_t w13_zrows[5] = {0, 0, 0, 0, 0};         // rows with W13_ZROW in their byte, per role of dtk_bench_gemv (dtk_w13_flagged_rows)
  uint64_t cached_image_key = 0;
  bool have_image = false;
  // ---- batched decode (dtk_*_slot / dtk_decode_batch_*): up to 64 decoding slots (+1) with their own KV
  int KVH = 0;                       // key/value heads (dtk_config.reserved[2]; 0 -> heads)
  int hd = 128;                      // decoder head dim: 128, or 64 (TinyLlama; no batched slots)
  bool proj_bias = true;             // mm_projector has a bias (v1) / bias-free connector (v2)
  int nb = 0;                        // number of batch slots (dtk_config.reserved[0])
  bool share_reads = true;           // forked slots read their shared prefix from the source slot (dtk_set_option "share_prefix_reads")
  int nt = 1;                        // 16-slot column tiles of the batched kernels (2 when nb > 17)
  std::vector<SeqHost> bseq;
  bf16_t* kvb = nullptr;             // [nb][L][2][H][Tmax][128]
  size_t kv_slot_stride = 0;
  // kv_format "mxfp8" (dtk_config.reserved[4] = 1): the MXFP8 shadow of the rows decode steps wrote, for the kv8_slots decoding slots
  // (prefix-cache slots never decode and have none).  Codes [kv8_slots][L][2][KVH][Tmax][128] u8 — the bf16 cache's own element
  // strides in bytes — and E8M0 scales [kv8_slots][L][2][KVH][Tmax][4].  Written by k_attn_tail_b<.., KV8> alone; poisoned (0xFF:
  // NaN as a code and as a scale) at dtk_create.  The bf16 cache stays the master of every row.
  int kv8 = 0; int kv8_slots = 0;
  uint8_t* kv8c = nullptr; uint8_t* kv8s = nullptr;
  bf16_t *xb = nullptr, *xnb = nullptr, *qb = nullptr, *aob = nullptr, *actb = nullptr;  // [16][d|ff]
  float* logits_b = nullptr;
  float* kpart = nullptr; unsigned* kctr = nullptr;   // k_gemv_bk / k_gemv_bkp partial sums + arrival counters
  int attn_nt = 1;             // batched attention: non-temporal loads of private K / V tiles (64 slots x 500 private keys: 7.14 -> 6.74 ms per step) (dtk_set_option "attn_nt")
  bool resid_kparts = true;    // batched N = d roles at 64 slots as two launches (k_gemv_bkp + k_resid_norm_b; measured 20.2 -> 21.2 rollouts/s): dtk_set_option("resid_kparts")
  float *pfx_m = nullptr, *pfx_l = nullptr, *pfx_o = nullptr;   // shared-prefix states [64][H][4] (+ x 128)
  int prefix_mfma = 0;               // shared prefixes (forks of one image) scored once per group of <= 16 slots on the matrix cores (k_attn_prefix_g); dtk_set_option "prefix_mfma".
                                     // Set at dtk_create from the context's size: 1 with 64 decoding slots, 0 below (see there)
  int pfx_splits = 4;                // key splits of that kernel (its grid z)
  int gqa_fused = 1;                 // batched attention: one block per (K/V head, slot) for GQA models
  int tail_threads = 256;            // block of k_attn_tail_b (rows per memory round trip = threads / 4); dtk_create: 128 with 64 decoding slots (the blocks then walk
                                     // private keys only and 2048 blocks of 2 waves are all resident), 256 below
  DecState* st_b = nullptr;          // [16]
  SamplingDev* sp_b = nullptr;       // [16]
  BatchState* bs_dev = nullptr;
  bf16_t* t_lm_head = nullptr;       // fragment-major copy of lm_head
  uint8_t* t8_lm_head = nullptr;     // fp8 pair-tiled copy of lm_head (weight_format fp8)
  // fp8 matrix-core step (kernels_batch_mx.hip; dtk_set_option "act_fp8"): the MFMA-family step of an fp8 model runs its GEMVs as
  // v_mfma_scale_f32_16x16x128_f8f6f4 on MXFP8 activations.  mx_ok = the model's shapes are covered and the buffers exist
  uint8_t* m_lm_head = nullptr;
  uint8_t *xn8 = nullptr, *xns = nullptr, *ao8 = nullptr, *aos = nullptr, *act8 = nullptr, *acts = nullptr;
  bool mx_ok = false;
  // act_fp8: 0 (default since round 5) = bf16 activations (fp8 weights widened in registers, bf16 MFMA: rounds 1-3); 1 = opt-in.  MXFP8
  // activations keep 3 mantissa bits: logits move ~1e-1 rel-L2 from the bf16-activation result (tests/test_gpu_parity_mx.py,
  // test_mxfp8_activations_against_bf16_activations), so the faster step is the caller's choice, not the library's.
  int act_fp8 = 0;
  bool launch_refused = false;       // a launcher of the step being issued had no kernel for its shape (nothing was launched for that role)
  bool tiled_ready = false;          // the fragment-major copies match the row-major weights
  bool ptiled_ready = false;         // ... and the prefill's own (LayerW::p_*)
  BatchState* bs_host = nullptr;     // pinned ring [DTK_MAX_INFLIGHT]
  SamplingDev* sp_stage = nullptr; uint32_t* draw_stage = nullptr;   // pinned [DTK_MAX_SLOTS]: per-slot set_sampling uploads queued on the stream
  DecState* st_stage = nullptr;      // pinned [DTK_MAX_SLOTS]: dtk_resume_slot's state upload (no stream sync: a slot is resumed again only sequences later)
  int64_t* tokb_dev = nullptr;       // [DTK_MAX_INFLIGHT][16]
  int64_t* tokb_host = nullptr;      // pinned mirror
  uint64_t blaunched = 0, bwaited = 0;
  hipEvent_t bstep_done[DTK_MAX_INFLIGHT] = {};
  // one captured step per column-tile count (1, 2, 4 tiles of 16 slots): a step only pays for the tiles up to its highest
  // active slot (32 trees on a 65-slot context run the 2-tile kernels)
  // (+ three more for the multi-vector step of a context with <= 5 slots: 1, 2 or 4 vectors)
  bool bgraph_ready[6] = {false, false, false, false, false, false};
  hipGraph_t bgraph[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipGraphExec_t bgraph_exec[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int nt_step = 1;                   // tile count of the step being launched / captured
  // Contexts with at most 5 slots (<= 4 decoding + a prefix slot: BASELINE config 4's 2 / 4 trees per rank at N = 8 / 4) decode
  // with the multi-vector kernels (kernels_decode_mv.hip): the single-sequence GEMVs carrying 1, 2 or 4 x vectors instead of a
  // 16-column MFMA tile.  The kernel family is a property of the CONTEXT (slot count at dtk_create, dtk_set_option "mv_slots"),
  // never of the active set, so a sequence's logits do not depend on which other slots happen to decode with it.
  int mv_slots = 4;                  // contexts with nb <= mv_slots + 1 use the family (0 = never)
  int mv_step = 0;                   // vectors of the step being launched / captured (0 = an MFMA step)
  int mv_tail_threads = 512;         // block of k_attn_tail_b in a multi-vector step (few blocks: more rows per round trip)
  dtk_sampling sampling{};
  SampleMB* smb = nullptr;           // multi-block sampler scratch (single sequence) / per slot
  SampleMB* smb_b = nullptr;
  bool mb_single = false;            // the captured single-sequence graph uses the multi-block sampler
  bool mb_batch = false;             // ... the batched graph
  bool slot_topk[DTK_MAX_SLOTS] = {};   // slots whose sampling needs top-k (single-block sampler only)
  bool slot_samples[DTK_MAX_SLOTS] = {}; // slots that sample (not greedy)
  // min_p / epsilon_cutoff (dtk_set_sampling_ext): which sampler instantiations the next captures must contain, and which the captured
  // graphs do contain (ensure_graph / ensure_batch_graph drop a graph of the other kind: a sequence with the values set again after
  // the reset of dtk_set_sampling keeps its graph)
  dtk_sampling_ext sampling_ext{};
  bool trunc_single = false, graph_trunc = false;
  bool slot_trunc[DTK_MAX_SLOTS] = {};
  bool trunc_batch = false, bgraph_trunc = false;
  // presence / frequency penalties (dtk_set_penalties): sequence 0 is the single one, 1 + slot a slot's.  Everything below is allocated
  // by the first call that sets a non-zero value (pen_alloc), so a context that never uses penalties allocates and launches nothing.
  // pen_single / pen_batch: which sampler instantiations the next captures must contain, graph_pen / bgraph_pen: which the captured graphs
  // do contain (as trunc_single / graph_trunc)
  uint16_t* pen_tab = nullptr;       // [1 + nb][pen_stride] count tables
  int pen_stride = 0;
  PenDev* pen_dev = nullptr;         // [1 + DTK_MAX_SLOTS]
  int32_t* pen_tok = nullptr;        // [1 + DTK_MAX_SLOTS] the step's sampled token, consumed by k_count_token (-1: nothing to count)
  int32_t* pen_ids_dev = nullptr;    // [1 + nb][Tmax] the ids a rebuild scatters
  int32_t* pen_ids_stage = nullptr;  // pinned mirror: a slot's rebuild is queued behind the step in flight, no drain
  PenDev* pen_stage = nullptr;       // pinned [1 + DTK_MAX_SLOTS]
  PenDev pen_val[1 + DTK_MAX_SLOTS] = {};   // the values as set
  int pen_start[1 + DTK_MAX_SLOTS] = {};    // penalty_start
  bool pen_single = false, graph_pen = false;
  bool pen_batch = false, bgraph_pen = false;
  // DRY (dtk_set_dry), indexed like the penalties: sequence 0 is the single one, 1 + slot a slot's.  Everything below is allocated by the
  // first call that sets a multiplier != 0 (dry_alloc, which also makes the penalties' records exist: DRY rides the PN samplers and shares
  // pen_tok and the trailing kernel), so a context that never uses DRY allocates and launches nothing.  dry_single / dry_batch and
  // graph_dry / bgraph_dry as pen_single / graph_pen
  uint8_t* dry_tab = nullptr;        // [1 + nb][dry_stride] match length per id, left by k_dry_scan for the step's sampler
  int dry_stride = 0;
  DryDev* dry_dev = nullptr;         // [1 + DTK_MAX_SLOTS]
  DryDev* dry_stage = nullptr;       // pinned [1 + DTK_MAX_SLOTS]
  int32_t* dry_hist = nullptr;       // [1 + nb][Tmax] the ids at positions [dry_start, next_pos)
  int32_t* dry_hist_stage = nullptr; // pinned mirror a rebuild fills
  DryLen* dry_len = nullptr;         // [1 + DTK_MAX_SLOTS]
  DryLen* dry_len_stage = nullptr;   // pinned
  int32_t* dry_touched = nullptr;    // [1 + nb][Tmax] the ids the last scan set
  int32_t* dry_ntouched = nullptr;   // [1 + DTK_MAX_SLOTS]
  DryDev dry_val[1 + DTK_MAX_SLOTS] = {};   // the records as set
  int dry_start[1 + DTK_MAX_SLOTS] = {};    // dry_start
  bool dry_live[1 + DTK_MAX_SLOTS] = {};    // the sequence's table / history may hold something (it has, or had, a multiplier)
  bool dry_single = false, graph_dry = false;
  bool dry_batch = false, bgraph_dry = false;
  // length control and logit bias (dtk_set_length_control / dtk_set_logit_bias), indexed like the penalties.  Everything below is allocated
  // by the first call that sets a value (len_alloc, which also makes the penalties' records exist: the rules ride the PN samplers), so a
  // context that never uses them allocates and launches nothing.  All of it is static for a sequence: nothing is rebuilt when the host
  // redefines one (the length comes from DecState::next_pos).  len_single / len_batch and graph_len / bgraph_len as pen_single / graph_pen
  LenDev* len_dev = nullptr;         // [1 + DTK_MAX_SLOTS]
  LenDev* len_stage = nullptr;       // pinned [1 + DTK_MAX_SLOTS]
  float* len_m = nullptr;            // [1 + nb][len_m_stride] the decay tables m[k]
  float* len_m_stage = nullptr;      // pinned mirror
  int len_m_stride = 0;              // Tmax + 1
  hipEvent_t len_m_up = nullptr;     // behind the last upload from len_m_stage: waited for before the mirror is written again
  double len_factor[1 + DTK_MAX_SLOTS] = {};          // the factor each decay table was built for (0: none yet)
  float* bias_tab = nullptr;         // [1 + nb][bias_stride] dense bias tables, 0 = no bias; the pairs travel as kernel arguments
  int bias_stride = 0;
  LenDev len_val[1 + DTK_MAX_SLOTS] = {};            // the records as set
  std::vector<int32_t> bias_ids[1 + DTK_MAX_SLOTS];  // the ids each table holds a value for
  bool len_single = false, graph_len = false;
  bool len_batch = false, bgraph_len = false;
  // classifier-free guidance (dtk_set_guidance): disjoint pairs of decoding slots.  cfg_n == 0: guidance_launch / follow_launch return
  // at once and the step launches what it launched before the feature existed.  The device table and the scratch are allocated by the
  // first call that forms a pair (hipMalloc of their own), so a context that never uses guidance allocates nothing.  Static for a
  // sequence, as length control: only dtk_set_guidance changes the table, and every change drops the captured batch steps — unless
  // dtk_reserve_guidance made the pairs standing: the three kernels then launch with cfg_res as their pair dimension whatever cfg_n is
  // (cfg_grid), entries [cfg_n, cfg_res) of the device table have cond = -1, and a change that fits only rewrites the table
  CfgPair cfg_pairs[DTK_MAX_BATCH / 2] = {};   // the pairs as set, [0, cfg_n)
  int cfg_n = 0;
  int cfg_res = 0;                   // dtk_reserve_guidance: pairs the captured steps are shaped for (0: none reserved, the grid is cfg_n)
  int64_t bgraph_captures = 0;       // captures of a batched step since creation (dtk_batch_graph_captures)
  CfgPair* cfg_dev = nullptr;        // [DTK_MAX_BATCH / 2]
  int32_t* cfg_forced = nullptr;     // [DTK_MAX_BATCH / 2] 1: the pair forwarded forced tokens in the last step (k_cfg_lse -> k_cfg_follow)
  float2* cfg_part = nullptr;        // [DTK_MAX_BATCH / 2][2][DTK_CFG_MAX_SLICES]
  float2* cfg_lse = nullptr;         // [DTK_MAX_BATCH / 2] (Lc, Lu) of the last step
  // prompt-lookup speculative decoding of slot 0 (dtk_spec_*): between dtk_spec_begin and dtk_spec_end the multi-vector step runs with
  // its vectors as consecutive positions of slot 0 (batch_step_launches_mv with spec_step set: the vectors' own DecStates, copies of
  // slot 0's SamplingDev, a device BatchState of its own, kv_slot_stride 0).  The steps share the batched steps' counters, events and
  // rings.  Everything below is one hipMalloc of the first dtk_spec_begin: a context that never speculates allocates nothing, and its
  // steps launch what they launched before.
  bool spec_on = false;
  bool spec_step = false;            // the step being launched / captured is a speculative one
  int spec_K = 0, spec_src = 0, spec_nv = 0;      // drafts per step, DTK_SPEC_LOOKUP | DTK_SPEC_TABLE, K + 1
  int spec_known_pos = 0;            // slot 0's length after the steps that have been waited for
  unsigned char* spec_mem = nullptr;
  SpecDev* spec_sd = nullptr;
  int32_t* spec_hist = nullptr;      // [Tmax]
  int32_t* spec_table = nullptr;     // [Tmax]
  DecState* spec_st = nullptr;       // [4]
  SamplingDev* spec_sp = nullptr;    // [4] copies of slot 0's record
  BatchState* spec_bs = nullptr;
  // the corpus of earlier programs (dtk_spec_set_corpus): one hipMalloc of the first non-empty call, [DTK_SPEC_CORPUS_MAX] ids and
  // [DTK_SPEC_CORPUS_BLOCKS] block results behind them.  spec_corpus_len > 0: a speculative step launches k_spec_corpus too
  int32_t* spec_corpus = nullptr;
  unsigned long long* spec_corpus_best = nullptr;
  int spec_corpus_len = 0;
  bool sgraph_ready[2] = {false, false};       // the captured speculative step with 2 / 4 vectors
  hipGraph_t sgraph[2] = {nullptr, nullptr};
  hipGraphExec_t sgraph_exec[2] = {nullptr, nullptr};
  uint64_t launched = 0, waited = 0;
  hipEvent_t step_done[DTK_MAX_INFLIGHT] = {};
  hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_c = nullptr;
  // dtk_vit_encode (the SelfSim reward's ViT passes) runs on its own stream so it overlaps with decode steps of other
  // sequences; the caller serialises it with prefills (they share the ViT activation buffers), see model/modeling.py
  hipStream_t stream_vit = nullptr;
  hipStream_t cur_stream = nullptr;   // stream of the GEMMs being issued (vit_forward sets it)
  hipEvent_t ev_va = nullptr, ev_vb = nullptr;
  hipEvent_t probe_a = nullptr, probe_b = nullptr;
  bool use_graph = true;
  bool graph_ready = false;
  hipGraph_t graph = nullptr, graph_short = nullptr;
  hipGraphExec_t graph_exec = nullptr, graph_short_exec = nullptr;
  int attn_full_max = 0;             // contexts below this use the one-block-per-head attention (measured slower: off)
  int attn_threads = 0;              // decode attention: 0 = k_attn_decode (contiguous key range per split), 256 | 512 | 1024 = k_attn_decode_t
  int attn_impl = 0;                 // prefill / ViT attention kernel: 0 auto, 1 VALU, 2 MFMA flash (dtk_set_option "attn_impl")
  bool gemm_naive = false;
  int probe = 0;
  bool probe_pending = false;
  dtk_stats stats{};
};

#define DTK_INTERNAL __attribute__((visibility("hidden")))

// sets the calling thread's error text (and the context's, or dtk_create's when c is null); returns code
DTK_INTERNAL int fail(dtk_ctx* c, int code, const char* fmt, ...);

#define HIPCHK(c, call)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail((c), DTK_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                  __FILE__, __LINE__);                                                    \
  } while (0)

DTK_INTERNAL size_t align_up(size_t x, size_t a);
DTK_INTERNAL uint16_t host_f2bf(float f);
DTK_INTERNAL float host_bf2f(uint16_t h);
DTK_INTERNAL float host_h2f(uint16_t h);

// ---- product helpers the op-level entry points share with the calls they stand for
DTK_INTERNAL int gelu_flag(const dtk_ctx* c);
DTK_INTERNAL int pen_check(dtk_ctx* c, float pp, float fp, int start, const char* who);
DTK_INTERNAL int dry_check(dtk_ctx* c, const dtk_dry* d, int V, const char* who);
DTK_INTERNAL DryDev dry_record(const dtk_dry* d);
DTK_INTERNAL int len_check(dtk_ctx* c, const dtk_length_ctl* l, int V, const char* who);
DTK_INTERNAL LenDev len_record(const dtk_length_ctl* l);
DTK_INTERNAL void len_table(double factor, float* m, int n);
DTK_INTERNAL int bias_check(dtk_ctx* c, const int32_t* ids, const float* values, int n, int V, const char* who);
DTK_INTERNAL int ext_check(dtk_ctx* c, const dtk_sampling_ext* x, const char* who);
struct ExtDev { int64_t qmin; float eps; };       // SamplingDev's tail
static_assert(offsetof(SamplingDev, eps) - offsetof(SamplingDev, qmin) == offsetof(ExtDev, eps) &&
              sizeof(SamplingDev) - offsetof(SamplingDev, qmin) == sizeof(ExtDev), "SamplingDev ends with (qmin, eps)");
DTK_INTERNAL ExtDev ext_dev(const dtk_sampling_ext* x);
DTK_INTERNAL void build_prefix_groups(BatchState* hb, const int32_t* active, bool enabled);
