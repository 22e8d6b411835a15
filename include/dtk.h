/*
 * dtk.h — C ABI of libdtk_hip.so, the MI355X (gfx950) image->TikZ decoder behind
 * DeTikZify's Python inference API.
 *
 * The reference (potamides/DeTikZify) has NO native/FFI seam: its boundary is the
 * duck-typed (model, processor) pair returned by detikzify.model.load
 * (reference detikzify/model/__init__.py:28-61) and consumed by
 * DetikzifyGenerator.generate (detikzify/infer/generate.py:209-227) and
 * ImageSim.from_detikzify (detikzify/evaluate/imagesim.py:61-89).  This header is
 * the C ABI that sits *underneath* that Python surface: each entry point names the
 * reference call it replaces.  Plain C, opaque handle, int status (0 = ok,
 * negative = error; text via dtk_last_error), caller-owned host buffers,
 * library-owned device buffers, one HIP stream per context.  A context is not
 * thread-safe, but may be driven from any one thread at a time (the reference
 * calls model.generate from a ThreadPool(1) worker, generate.py:248-258);
 * contexts are independent -> one context per GPU / rank.
 */
#ifndef DTK_H
#define DTK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DTK_ABI_VERSION 7   /* 2: batch arrays of 32 entries (were 16); 3: DTK_MAX_BATCH = 64; 4: dtk_max_decode_slots,
                             * contexts with <= 5 slots decode in slots 0..3 (multi-vector kernels);
                             * 5: dtk_op_gemv_mx, dtk_mx_layout, dtk_stats.last_batch_step_fp8_mfma;
                             * 6: dtk_engine_* (the native run loop of a batch; replaces ABI 4's dtk_decode_batch_run), dtk_max_positions; dtk_last_error is
                             * per calling thread; 7: the TikZero adapter (dtk_adapter_*, *_text variants, dtk_op_gemm_gated) */

typedef struct dtk_ctx dtk_ctx;

enum { DTK_F32 = 0, DTK_BF16 = 1, DTK_F16 = 2 };

enum {
  DTK_OK = 0,
  DTK_ERR_ARG = -1,     /* bad argument / shape / unknown tensor name          */
  DTK_ERR_HIP = -2,     /* a HIP runtime call failed                            */
  DTK_ERR_STATE = -3,   /* call sequence violated (e.g. decode before prefill)  */
  DTK_ERR_RANGE = -4    /* context length would exceed max_positions            */
};

/* Architecture of one checkpoint.  Decoder fields are HF LlamaConfig fields
 * (read from the checkpoint's config.json, never hard-coded; reference
 * detikzify/model/v1/configuration_detikzify.py:3-13).  Vision fields describe the
 * timm ViT created at detikzify/model/v1/modeling_detikzify.py:94. */
typedef struct dtk_config {
  /* LLaMA decoder */
  int32_t hidden;          /* d                                   */
  int32_t layers;          /* L                                   */
  int32_t heads;           /* H query heads (kv heads: reserved[2]) */
  int32_t head_dim;        /* hd: 128, or 64 (no batch slots)      */
  int32_t ffn;             /* intermediate_size                   */
  int32_t vocab;           /* V                                   */
  int32_t max_positions;   /* KV capacity in tokens (<= 2048 for v1, generate.py:383) */
  float   rms_eps;
  float   rope_theta;
  float   rope_factor;     /* linear RoPE scaling factor (1 = none) */
  /* vision tower (timm vit_so400m_patch14_siglip_384 family) */
  int32_t vit_dim;         /* D (1152)                            */
  int32_t vit_depth;       /* 27                                  */
  int32_t vit_heads;       /* 16 -> head dim 72                   */
  int32_t vit_mlp;         /* 4304                                */
  int32_t vit_patch;       /* 14                                  */
  int32_t vit_image;       /* 384                                 */
  int32_t vit_feature_layer; /* block index whose output feeds the LM (modeling_detikzify.py:104) */
  float   vit_ln_eps;      /* 1e-6                                */
  int32_t vit_gelu_tanh;   /* 0 = erf GELU (timm default), 1 = tanh approximation */
  /* glue */
  int32_t concat_patches;  /* 3  (modeling_detikzify.py:101)       */
  int32_t image_token_id;  /* == BOS for v1 (v1/__init__.py:49)    */
  int32_t attn_splits;     /* split-K factor of decode attention; 0 = default */
  int32_t reserved[7];     /* [0] = batch slots for dtk_decode_batch_* (0 = none)
                            * [1] = weight format of the decoder's Linear weights: 0 bf16; 1 = fp8 e4m3 + per-row 2^e scales; 2 = OCP MXFP4
                            *       (E2M1 codes + one E8M0 scale per 32 weights along K) for q/k/v, o, gate/up and down of every layer, fp8 for
                            *       lm_head; single-sequence decode only: with [0] > 0 dtk_create fails with DTK_ERR_ARG.  Quantised on the
                            *       device at load; the bf16 tensors are overwritten with the de-quantised (effective) weights
                            * [2] = key/value heads (GQA, num_key_value_heads); 0 = heads (MHA, all v1 models)
                            * [3] = architecture flags, DTK_ARCH_*
                            * [4] = key/value row format of the batched and multi-vector decode steps: 0 = bf16; 1 = the rows that DECODE STEPS
                            *       wrote are also kept as OCP MXFP8 (E4M3 codes + one E8M0 scale per 32 dims of a head's row: 132 bytes where the
                            *       bf16 row has 256) in shadow planes that only the batched attention kernel writes, and those steps read them
                            *       from there.  The bf16 cache stays the master of every row and every other reader (prefill, scoring, forks,
                            *       the single-sequence step, dtk_read_tensor) keeps reading it: the format COSTS memory (+0.516 x the bf16 cache
                            *       of every decoding slot) and buys attention bandwidth.  Needs [0] > 0; any other value, or 1 with [0] == 0,
                            *       fails dtk_create with DTK_ERR_ARG before anything is allocated.  See dtk_kv8_info.              */
} dtk_config;
/* v2 connector (reference detikzify/model/modeling_detikzify.py:62-70): Linear(concat*D -> d, bias=False) */
#define DTK_ARCH_PROJ_NO_BIAS 1

/* Per-generation sampling state: the HF logits processors + sampler that
 * DetikzifyGenerator.generate configures (generate.py:218-227; HF
 * generation/utils.py _sample, logits_process.py:300-303,528-540,1395,1860-1866). */
typedef struct dtk_sampling {
  int32_t do_sample;       /* 0 = greedy argmax, 1 = multinomial                     */
  float   temperature;     /* used when do_sample                                    */
  float   top_p;           /* nucleus; 1.0 disables                                  */
  int32_t top_k;           /* 0 disables                                             */
  uint64_t seed;           /* counter-based RNG key; draw n uses counter n           */
  int32_t n_bad;           /* banned single-token ids (bad_words_ids=[[id]])         */
  int32_t bad_ids[8];
  int32_t n_begin_suppress;/* ids suppressed only for the first generated token      */
  int32_t begin_suppress_ids[8];
  int32_t n_always_suppress; /* extra ids banned at every step (fixed-work benches)  */
  int32_t always_suppress_ids[8];
} dtk_sampling;

/* The two HF warpers behind top-p (additive, ABI 7; dtk_set_sampling_ext): MinPLogitsWarper and EpsilonLogitsWarper as thresholds on
 * the sampler's integer masses q_i = floor(exp(z_i - zmax) * 2^31).  Both 0 = off. */
typedef struct dtk_sampling_ext {
  float   min_p;           /* [0, 1]: keep q_i >= (int64)((double)min_p * 2^31), i.e. p_i >= min_p * p_max (the maximum always stays)     */
  float   epsilon_cutoff;  /* [0, 1): keep q_i >= (int64)((double)eps * (double)total_m), total_m = the mass kept after top-k, top-p and
                            * min-p; if nothing is left: the first arg-max alone                                                         */
  int32_t reserved[6];     /* zero                                                                                                       */
} dtk_sampling_ext;

typedef struct dtk_stats {
  uint64_t weight_bytes_per_token;  /* W: decoder layers + final norm + lm_head       */
  uint64_t kv_bytes_per_ctx_token;  /* K: 2*L*d*sizeof(bf16)                          */
  uint64_t decode_steps;            /* decode-step launches since create              */
  uint64_t prefill_tokens;          /* tokens pushed through the batched prefill      */
  uint64_t vit_images;              /* images encoded                                 */
  double   last_prefill_ms;         /* device time of last dtk_prefill / dtk_score (HIP events) */
  double   last_vit_ms;             /* ViT part of it                                 */
  double   probe_kernel_ms_sum;     /* in-graph event probe around the gate/up GEMV of the middle layer */
  uint64_t probe_kernel_launches;
  uint64_t probe_kernel_bytes;      /* algorithmic bytes of one such launch           */
  double   probe_event_pair_ms;     /* elapsed time of an EMPTY hipEventRecord pair on the stream (the fixed cost inside every
                                     * probe interval; calibrated when probe mode is switched on)            */
  uint32_t last_batch_step_slots;   /* slots the kernels of the last dtk_decode_batch_launch computed: 1 | 2 | 4 (multi-vector
                                     * kernels) or 16 | 32 | 64 (one, two, four MFMA column tiles)            */
  uint32_t device_errors;           /* sticky: in-kernel protocol timeouts seen so far (a ring hand-off that expired); any
                                     * non-zero value makes dtk_decode_batch_wait fail                          */
  uint32_t last_batch_step_fp8_mfma; /* 1: the last dtk_decode_batch_launch ran the fp8 matrix-core kernels (MXFP8 activations,
                                     * option "act_fp8"), 0: the bf16-activation kernels                        */
  uint32_t w13_counts;              /* bf16 contexts with option "w13": what the packer of the 13-bit weight planes found, valid once a
                                     * single-sequence step has run: bits 0-9 matrices with planes, 10-19 matrices left as bf16 (an
                                     * unpackable row), 20-31 unpackable rows (saturating at 4095); 0 otherwise (was reserved0)  */
} dtk_stats;

int  dtk_abi_version(void);
/* layout check for bindings: sizeof of 0 dtk_config, 1 dtk_sampling, 2 dtk_stats; offsetof of 3 dtk_sampling.seed,
 * 4 dtk_config.reserved, 5 dtk_stats.probe_event_pair_ms; sizeof of 6 dtk_join, 7 dtk_engine_stats, 8 dtk_engine_ops; offsetof of
 * 9 dtk_join.sampling, 10 dtk_join.error_out; sizeof of 11 dtk_adapter_config, 12 dtk_sampling_ext; -1 for anything else */
int  dtk_abi_struct_size(int which);
/* last error of a context; ctx may be NULL for the error of a failed dtk_create */
const char* dtk_last_error(const dtk_ctx* ctx);

/* Lifetime.  Allocates every weight, activation and KV buffer up front
 * (replaces DetikzifyForCausalLM.from_pretrained + initialize_vision_modules,
 * reference v1/__init__.py:35-54). */
int  dtk_create(const dtk_config* cfg, int device, dtk_ctx** out);
void dtk_destroy(dtk_ctx* ctx);

/* Weights.  Names are the checkpoint's state-dict keys: HF Llama keys
 * ("model.layers.3.self_attn.q_proj.weight", "model.embed_tokens.weight",
 * "model.norm.weight", "lm_head.weight", "model.mm_projector.weight|bias") and
 * timm ViT keys prefixed "vision_model." ("vision_model.blocks.0.attn.qkv.weight",
 * "vision_model.attn_pool.latent", ...).  Host data may be f32/bf16/f16; storage is bf16. */
int  dtk_load_tensor(dtk_ctx* ctx, const char* name, const void* host, int dtype,
                     const int64_t* shape, int ndim);
/* copy a stored tensor (bf16, same logical shape as the checkpoint tensor) back to the host */
int  dtk_read_tensor(dtk_ctx* ctx, const char* name, void* host_out_bf16, int64_t n_elems);
/* deterministic synthetic weights generated on the device (no real checkpoints
 * exist offline); bit-identical to oracle/synth.py for the same seed. */
int  dtk_fill_synthetic(dtk_ctx* ctx, uint64_t seed);
/* number of tensor names / i-th name / element count (for loaders and tests) */
int  dtk_num_tensors(const dtk_ctx* ctx);
const char* dtk_tensor_name(const dtk_ctx* ctx, int i);
int64_t dtk_tensor_numel(const dtk_ctx* ctx, const char* name);

/* Vision tower: replaces DetikzifyVisionModel.forward / get_intermediate_layers
 * (reference v1/modeling_detikzify.py:63-72).  pixels: B x 3 x S x S fp32 NCHW
 * (host).  feats_out: B x N x D bf16 (post final-LayerNorm features of the
 * configured feature layer = get_intermediate_layers(n=[layer], norm=True)), pooled_out: B x D bf16 (MAP head), either
 * may be NULL.  With pooled_out the call is DetikzifyVisionModel.forward and feats_out receives its last_hidden_state
 * (forward_features: all blocks + final norm; the same tensor unless feature_layer != depth - 1).  Requesting
 * pooled_out from a context whose attn_pool tensors were never loaded is DTK_ERR_STATE. */
int  dtk_vit_encode(dtk_ctx* ctx, const float* pixels, int batch,
                    void* feats_out_bf16, void* pooled_out_bf16);

/* Prefill: replaces DetikzifyForCausalLM.forward with input_ids.shape[1] != 1
 * (reference v1/modeling_detikzify.py:144-200,218-257).  ids: T int64 (host);
 * pixels (1x3xSxS fp32 host) may be NULL when the ids contain no image tokens or
 * when image_key matches the previously encoded image.  flags: DTK_PREFILL_*.
 * logits_last_out (V fp32, host) may be NULL.  Afterwards the context holds KV
 * for T positions and the logits of position T-1. */
#define DTK_PREFILL_REUSE_PREFIX 1   /* keep KV of the longest common prefix with the cached ids */
#define DTK_PREFILL_REUSE_IMAGE  2   /* skip the ViT when image_key equals the cached key        */
int  dtk_prefill(dtk_ctx* ctx, const int64_t* ids, int T, const float* pixels,
                 uint64_t image_key, int flags, float* logits_last_out);

/* Scoring: log p(ids[t] | ids[:t], image) for t = first .. T-1 in ONE pass — the teacher-forced half of
 * DetikzifyForCausalLM.forward(input_ids, pixel_values, labels) (reference v1/modeling_detikzify.py:260-271,
 * modeling_detikzify.py:361-376: logits of every position, shifted cross-entropy).  Runs the prefill of the same arguments
 * (flags: DTK_PREFILL_*; prefix reuse stops at position first-1, whose hidden state is the first one scored) and leaves the
 * context exactly as dtk_prefill does — KV, cached ids, last-row logits — so dtk_decode may continue from it.  Then the final
 * norm and lm_head run over rows first-1 .. T-2 on the matrix cores with the log-softmax folded into the GEMM's epilogue: no
 * [T][V] logits exist; a row's logits are the values dtk_prefill's last-row path gives (bf16-rounded), exp / log in fp32.
 * 1 <= first <= T-1, T >= 2.  logprob_out [T-first]; argmax_out (the greedy token of each position, lowest id on ties) and
 * lse_out (logsumexp of the row) [T-first] or NULL.  The first call allocates a workspace of max_positions x ceil(V/128) x
 * 16 bytes that the context keeps. */
int  dtk_score(dtk_ctx* ctx, const int64_t* ids, int T, const float* pixels, uint64_t image_key, uint32_t flags,
               int first, float* logprob_out, int32_t* argmax_out, float* lse_out);

/* Scoring N candidate continuations of ONE prompt in one packed pass: log p(cand_i[j] | prefix, cand_i[:j]) for every candidate i and
 * token j — what N calls of dtk_score(prefix + cand_i, first = P) give, for one stream of the decoder's weights instead of N.
 * prefix_ids [P >= 1]: the prompt (image placeholders + text; pixels / image_key / flags as dtk_prefill).  cand_ids: the candidates
 * concatenated, cand_len [N]: their lengths (each >= 1, N >= 1).  logprob_out, and argmax_out / lse_out or NULL: sum(cand_len) entries
 * in the same order.  The pass runs the prompt's positions lcp .. P-2 (lcp = the longest common prefix with the cached sequence when
 * DTK_PREFILL_REUSE_PREFIX is set, at most P-1) and one segment of len_i rows per candidate — inputs prefix[P-1], cand_i[0 .. len_i-2]
 * at positions P-1 + j, K / V at cache rows P-1 + len_0 + .. + len_{i-1} + j; a row sees the prompt and the rows of its own segment up
 * to itself.  Capacity: P-1 + sum(cand_len) <= max_positions, else DTK_ERR_RANGE.  Every argument is checked before anything is
 * launched and a refused call leaves the context untouched; DTK_ERR_STATE under dtk_set_option("attn_impl", 1) (the VALU attention
 * kernel has no segmented form).  The image placeholders must lie in the prompt: when an image is in use (pixels, or the cached image
 * of image_key with DTK_PREFILL_REUSE_IMAGE) a candidate that holds image_token_id is refused with dtk_prefill's message for a wrong
 * number of image tokens; without an image the id is a token like any other, as in dtk_score.
 * Afterwards the context holds the prompt's first P-1 positions (cached ids, image key, K / V rows [0, P-1)), which a following
 * dtk_prefill / dtk_score / dtk_score_packed with DTK_PREFILL_REUSE_PREFIX reuses, and NO current sequence: dtk_decode /
 * dtk_decode_launch return DTK_ERR_STATE until the next prefill.  stats.last_prefill_ms / prefill_tokens count the pass as a
 * prefill's.  The first call allocates dtk_score's workspace (max_positions rows: P = 1 leaves every row to the candidates) and
 * 24 x max_positions bytes of row tables that the context keeps. */
int  dtk_score_packed(dtk_ctx* ctx, const int64_t* prefix_ids, int P, const float* pixels, uint64_t image_key, uint32_t flags,
                      const int64_t* cand_ids, const int32_t* cand_len, int N,
                      float* logprob_out, int32_t* argmax_out, float* lse_out);

/* Sampling configuration for the following decode calls (resets the draw counter). */
int  dtk_set_sampling(dtk_ctx* ctx, const dtk_sampling* s);

/* Decode: one call = one iteration of HF GenerationMixin._sample (logits
 * processors -> argmax|multinomial on the pending logits -> append -> forward of
 * the new token), hipGraph-replayed.  dtk_decode_launch enqueues a step without
 * waiting; dtk_decode_wait returns the oldest un-read token (at most
 * DTK_MAX_INFLIGHT steps may be pending).  dtk_decode = launch + wait. */
#define DTK_MAX_INFLIGHT 4
#define DTK_VIT_BATCH 8      /* images dtk_vit_encode runs as one pass over the tower (larger batches: several passes) */
int  dtk_decode_launch(dtk_ctx* ctx);
int  dtk_decode_wait(dtk_ctx* ctx, int64_t* token_out);
int  dtk_decode(dtk_ctx* ctx, int64_t* token_out);
/* logits (V fp32) the next sampling step will consume, copied to the host */
int  dtk_get_logits(dtk_ctx* ctx, float* logits_out);
/* current context length (tokens with KV) */
int  dtk_context_len(const dtk_ctx* ctx);
/* 1 = replay the decode step as a hipGraph (default), 0 = plain launches */
int  dtk_set_graph_mode(dtk_ctx* ctx, int enabled);
int  dtk_synchronize(dtk_ctx* ctx);
int  dtk_get_stats(dtk_ctx* ctx, dtk_stats* out);

/* Batched decode for independent rollouts of one GPU: dtk_config.reserved[0] = number
 * of slots (<= DTK_MAX_SLOTS), each with its own KV cache, sampling state and logits.  One
 * dtk_decode_batch_* step = one _sample iteration for every active slot with ONE pass over the weights
 * (bytes/step = W + sum_b K*t_b).  Up to 5 slots: slots 0..3 decode with the multi-vector kernels (the single-sequence GEMVs
 * carrying 1, 2 or 4 input vectors: BASELINE config 4 leaves 2 / 4 trees per rank at N = 8 / 4, reference examples/eval.py:80-83);
 * 6..17 slots: slots 0..15 decode (one 16-column MFMA tile); 18..33 slots:
 * slots 0..31 decode (two tiles); 34..72 slots: slots 0..63 decode (four tiles); slots beyond the decoding ones can only be
 * prefilled / forked from (prefix cache: one per image in flight — BASELINE config 5 runs 8 images on one GPU).
 * The `active` / `tokens_out` arrays always have DTK_MAX_BATCH entries.
 * The image embeddings cache is shared (DTK_PREFILL_REUSE_IMAGE). */
#define DTK_MAX_BATCH 64
#define DTK_MAX_SLOTS (DTK_MAX_BATCH + 8)
int  dtk_num_slots(const dtk_ctx* ctx);
/* how many slots (0 .. n-1) may take part in a decode step: 4, 16, 32 or 64, at most dtk_num_slots */
int  dtk_max_decode_slots(const dtk_ctx* ctx);
int  dtk_prefill_slot(dtk_ctx* ctx, int slot, const int64_t* ids, int T, const float* pixels,
                      uint64_t image_key, int flags, float* logits_last_out);
int  dtk_set_sampling_slot(dtk_ctx* ctx, int slot, const dtk_sampling* s);
int  dtk_decode_batch_launch(dtk_ctx* ctx, const int32_t* active /* [DTK_MAX_BATCH] */);
int  dtk_decode_batch_wait(dtk_ctx* ctx, int64_t* tokens_out /* [DTK_MAX_BATCH] */);
int  dtk_kv_fork(dtk_ctx* ctx, int src_slot, int dst_slot, int n_tokens);   /* share a prefix's KV (f1) */
/* f1, same-slot reuse for returning MCTS trees (reference infer/generate.py:305-353 re-prefills the path to the selected node
 * on every rollout): dtk_slot_lcp = how many leading tokens of `ids` the slot's KV cache still holds (prefilled or decoded, same
 * image key); dtk_resume_slot = continue from there WITHOUT a prefill when all but the last prompt token are cached — the next
 * batched step forwards ids[T-1] for this slot instead of sampling and returns it as that step's token (the caller drops it),
 * the step after samples the first new token. */
int  dtk_slot_lcp(dtk_ctx* ctx, int slot, const int64_t* ids, int n_tokens, uint64_t image_key, int* lcp_out);
int  dtk_resume_slot(dtk_ctx* ctx, int slot, const int64_t* ids, int n_tokens, uint64_t image_key);
int  dtk_slot_cached_ids(dtk_ctx* ctx, int slot, int64_t* ids_out, int n_max);   /* diagnostic: what the slot's cache holds; returns the count */
int  dtk_get_logits_slot(dtk_ctx* ctx, int slot, float* logits_out);
int  dtk_context_len_slot(const dtk_ctx* ctx, int slot);
/* kv_format mxfp8 (dtk_config.reserved[4] = 1; additive, ABI 7).  Every slot has a boundary kv8_from: a batched step of the slot at
 * position pos reads rows [.., kv8_from) in bf16 as a bf16 context does and rows [kv8_from, pos) from the shadow; row pos, which the
 * step's q/k/v launch has just written in bf16, is quantised by the attention kernel (groups of 32 dims: e = the smallest exponent with
 * amax * 2^-e <= 448, codes = e4m3(x * 2^-e) — oracle.llama.mx_quantise bit for bit), scored from the de-quantised values code * 2^e,
 * and stored, so a row contributes the same numbers in the step that writes it and in every later one.  The boundary is set to the
 * slot's new length by every prefill into it (with prefix reuse too: all of [0, T) then counts as prefill rows) and to n_tokens by
 * dtk_kv_fork for the destination (nothing of the shadow is copied: shared rows are bf16 rows); dtk_resume_slot replaces it by
 * min(kv8_from, T - 1), so the rows the slot decoded earlier and keeps stay MXFP8 rows.
 *   dtk_kv8_info: the slot's boundary; DTK_ERR_STATE in a bf16 context.
 *   dtk_read_kv8: diagnostic — rows [row0, row0 + nrows) of layer `layer`, which = 0 keys | 1 values, of a decoding slot, all kv heads:
 *                 codes_out [KVH][nrows][128], scales_out [KVH][nrows][4] (E8M0) and the bf16 rows beside them bf16_out [KVH][nrows][128];
 *                 any of the three may be NULL.  Shadow rows no step has written hold 0xFF.  Waits for the launched steps. */
int  dtk_kv8_info(dtk_ctx* ctx, int slot, int* from_out);
int  dtk_read_kv8(dtk_ctx* ctx, int slot, int layer, int which, int row0, int nrows, uint8_t* codes_out, uint8_t* scales_out, uint16_t* bf16_out);

int  dtk_max_positions(const dtk_ctx* ctx);               /* KV capacity of a sequence in tokens (dtk_config.max_positions) */

/* ---- Text conditioning: the TikZero cross-attention adapter (ABI 7) ---------------------------------------------------------------
 * Replaces CrossAttentionAdapterMixin.load_cross_attn_adapter / add_hooks (reference detikzify/model/adapter/modeling_adapter.py,
 * loaded by detikzify/model/__init__.py:58-59).  An embedding model (a LlamaModel without head: Llama-3.2-1B, hd 64, GQA) turns the
 * text into final-norm hidden states; Linear(d_emb -> D, bias) connects them to the tower; before every ViT block i with
 * (i + 1) % every_n == 0 a CrossAttentionLayer runs:
 *   x = x + bf16(sigmoid(attn_gate)) * out_proj(attn(q_norm(q_proj(LN1(x))), k_norm(k_proj(c)), v_proj(c)))
 *   x = x + bf16(sigmoid(mlp_gate)) * fc2(gelu(fc1(LN2(x))))                    (q_norm / k_norm: LayerNorm per head, eps = vit_ln_eps)
 * Only the HF SigLIP tower of a v2 checkpoint has these hooks: dtk_adapter_create refuses a v1 context (DTK_ERR_ARG, "Couldn't
 * locate vision encoder layers!", the reference's own refusal).  Tensors are registered with dtk_load_tensor / dtk_read_tensor /
 * dtk_fill_synthetic under the reference's state-dict names: "embedding_model.embed_tokens.weight", "embedding_model.layers.3.
 * self_attn.q_proj.weight", "embedding_model.norm.weight" (+ "embedding_model.rope.cos|sin", the embedding model's RoPE tables),
 * "adapter.connector.weight|bias", "adapter.dummy_input", "adapter.layers.5.cross_attn.q_norm.weight",
 * "adapter.layers.5.cross_attn_attn_gate", ...  The connector output and every cross layer's k / v (after k_norm) are computed once
 * per text and kept for later calls with the same text ids (one text at a time; the cache compares the ids themselves, text_key
 * only keys the image prefixes below).
 * Text variants: text_ids (T_text int64, 1 <= T_text <= text_max, no padding) condition the tower; pixels = NULL means the adapter's
 * dummy input (dummy_input.clamp(-1, 1)) for every image.  The KV prefix and image caches of the *_text prefills are keyed by the
 * pair (image_key, text_key): the same pixels under another text are another image.  text_key 0 = unknown (never reused). */
typedef struct dtk_adapter_config {
  int32_t every_n;         /* cross_attn_every_n_layers (>= 1)                                  */
  int32_t text_max;        /* longest text in tokens (tokenizer model_max_length: 512)          */
  /* the embedding model (HF LlamaConfig fields) */
  int32_t hidden, layers, heads, kv_heads, head_dim, ffn, vocab;
  float   rms_eps;
  float   rope_theta;      /* RoPE tables are loaded as "embedding_model.rope.cos|sin"; these seed the default (unscaled) ones */
  float   rope_factor;
  float   rope_low_freq_factor, rope_high_freq_factor;
  int32_t rope_original_max_position;
  int32_t reserved[3];
} dtk_adapter_config;
int  dtk_adapter_create(dtk_ctx* ctx, const dtk_adapter_config* cfg);
int  dtk_adapter_destroy(dtk_ctx* ctx);          /* unload_cross_attn_adapter: image-only calls are as if it never existed */
int  dtk_has_adapter(const dtk_ctx* ctx);
int  dtk_vit_encode_text(dtk_ctx* ctx, const float* pixels, int batch, const int64_t* text_ids, int T_text, uint64_t text_key,
                         void* feats_out_bf16, void* pooled_out_bf16);
int  dtk_prefill_text(dtk_ctx* ctx, const int64_t* ids, int T, const float* pixels, uint64_t image_key,
                      const int64_t* text_ids, int T_text, uint64_t text_key, int flags, float* logits_last_out);
int  dtk_prefill_slot_text(dtk_ctx* ctx, int slot, const int64_t* ids, int T, const float* pixels, uint64_t image_key,
                           const int64_t* text_ids, int T_text, uint64_t text_key, int flags, float* logits_last_out);
/* dtk_score with the tower conditioned on text_ids (as dtk_prefill_text; pixels = NULL: the adapter's dummy input) */
int  dtk_score_text(dtk_ctx* ctx, const int64_t* ids, int T, const float* pixels, uint64_t image_key,
                    const int64_t* text_ids, int T_text, uint64_t text_key, uint32_t flags,
                    int first, float* logprob_out, int32_t* argmax_out, float* lse_out);
/* dtk_score_packed with the tower conditioned on text_ids (as dtk_score_text) */
int  dtk_score_packed_text(dtk_ctx* ctx, const int64_t* prefix_ids, int P, const float* pixels, uint64_t image_key,
                           const int64_t* text_ids, int T_text, uint64_t text_key, uint32_t flags,
                           const int64_t* cand_ids, const int32_t* cand_len, int N,
                           float* logprob_out, int32_t* argmax_out, float* lse_out);
/* diagnostic: the embedding model's last_hidden_state (T_text x hidden bf16) of text_ids */
int  dtk_adapter_embed(dtk_ctx* ctx, const int64_t* text_ids, int T_text, void* hidden_out_bf16);
/* the key the *_text prefills cache an image prefix under (image_key, text_key) -> key; 0 when either is 0 */
uint64_t dtk_text_image_key(uint64_t image_key, uint64_t text_key);

/* ---- The run loop of a batch of rollouts, native (ABI 6) ------------------------------------------------------------------------
 * Replaces, for every sequence decoded in a slot, the per-token host iteration of HF GenerationMixin._sample
 * (generation/utils.py:2875-2936) that DetikzifyGenerator.generate runs in a worker thread and consumes line by line
 * (reference detikzify/infer/generate.py:246-282): ONE native thread per engine launches and collects the batched steps — two in
 * flight, so the device never waits for the host — appends every slot's token to that slot's ring, applies the sequence's own stop
 * rules (stop ids = EOS, token budget = max_length) and wakes the slot's reader only when a FLUSH token (the caller's newline table),
 * `flush_max` tokens or the end of the sequence has arrived.  Callers block in dtk_engine_read (no interpreter lock held) and are
 * woken once per source line instead of once per token; joins and leaves are queued and executed by the same thread between steps,
 * so nothing but that thread ever touches the context's main stream.  A slot's tokens do not depend on which other slots decode
 * next to it, so a sequence is the same ids as through dtk_decode_batch_launch / _wait driven from the host.
 * dtk_engine_create drives `ctx` (which must outlive the engine and must not be used for prefill / decode calls by anybody else
 * meanwhile; dtk_vit_encode from other threads stays legal: own stream, serialised with image prefills inside the library).
 * dtk_engine_create_ops drives a caller-supplied device (the CPU tests' scripted device: tests/test_native_engine.py). */
typedef struct dtk_engine dtk_engine;
typedef struct dtk_engine_ops {      /* the device under the loop: same contracts as the dtk_* entry points of the same names */
  void* dev;
  int (*launch)(void* dev, const int32_t* active /* [DTK_MAX_BATCH] */);
  int (*wait)(void* dev, int64_t* tokens_out /* [DTK_MAX_BATCH] */);
  int (*prefill_slot)(void* dev, int slot, const int64_t* ids, int T, const float* pixels, uint64_t image_key, int flags);
  int (*set_sampling_slot)(void* dev, int slot, const dtk_sampling* s);
  int (*kv_fork)(void* dev, int src_slot, int dst_slot, int n_tokens);
  int (*slot_lcp)(void* dev, int slot, const int64_t* ids, int n_tokens, uint64_t image_key, int* lcp_out);
  int (*resume_slot)(void* dev, int slot, const int64_t* ids, int n_tokens, uint64_t image_key);
  int (*context_len_slot)(void* dev, int slot);
  const char* (*last_error)(void* dev);
  int32_t max_positions;
  int32_t decode_slots;
} dtk_engine_ops;

/* how a join got its prompt into the slot (dtk_join.how_out) */
enum { DTK_JOIN_FULL = 0,        /* whole prompt prefilled (ViT included unless the image is cached)                  */
       DTK_JOIN_FORK_TAIL = 1,   /* image prefix forked from prefix_src, what follows prefilled                       */
       DTK_JOIN_FORK_WHOLE = 2,  /* prompt == prefix: KV and next-token logits forked, nothing computed                */
       DTK_JOIN_RESUMED = 3,     /* the slot still held all but the last prompt token: continued in place, no prefill */
       DTK_JOIN_IN_PLACE = 4 };  /* the slot still held the image prefix: only what follows prefilled                 */
/* sequence states (dtk_engine_read state_out) */
enum { DTK_SEQ_RUNNING = 1, DTK_SEQ_FINISHED = 2 /* stop id or budget */, DTK_SEQ_LEFT = 3 /* dtk_engine_leave / engine destroyed */ };

typedef struct dtk_join {
  int32_t slot;                  /* decoding slot of the sequence; with n_candidates > 0: the slot taken when no candidate can resume */
  int32_t n_ids;
  const int64_t* ids;            /* the whole prompt (host)                                                                        */
  const float* pixels;           /* 1 x 3 x S x S fp32 (host) or NULL, as dtk_prefill_slot                                         */
  uint64_t image_key;
  int32_t try_resume;            /* 1: dtk_resume_slot when the slot's cache holds ids[0, n_ids - 1) (an MCTS tree coming back)     */
  int32_t n_candidates;          /* > 0 (with try_resume): resume in the candidate with the longest such match (lowest index on ties) */
  int32_t candidates[DTK_MAX_BATCH];
  int32_t prefix_len;            /* leading ids that are the shareable image prefix; 0 = no sharing: a full prefill with full_flags */
  int32_t prefix_src;            /* slot to fork the prefix from (-1: none)                                                         */
  int32_t prefix_src_whole;      /* 1: prefix_src is a prefix-cache slot (holds exactly the prefix + its next-token logits)         */
  int32_t prefix_encode;         /* 1: first prefill ids[0, prefix_len) + pixels into prefix_src (greedy), then fork                */
  int32_t prefix_in_place;       /* 1: `slot` itself still holds the prefix: prefill with DTK_PREFILL_REUSE_*                       */
  int32_t full_flags;            /* DTK_PREFILL_* of the full prefill                                                               */
  dtk_sampling sampling;
  int32_t max_new_tokens;        /* token budget of the sequence (max_length - n_ids)                                               */
  int32_t n_stop;
  int64_t stop_ids[8];           /* the sequence ends WITH the first of these it emits (EOS)                                        */
  int32_t flush_mode;            /* 0: every token wakes the reader; 1: flush tokens (dtk_engine_set_flush_tokens) / flush_max      */
  int32_t flush_max;             /* mode 1: wake the reader after at most this many undelivered tokens (0 = 64)                     */
  int32_t slot_out;              /* out: the slot the sequence decodes in                                                           */
  int32_t how_out;               /* out: DTK_JOIN_*                                                                                 */
  char    error_out[240];        /* out: text of a failed join (the engine itself stays usable unless the device failed)            */
} dtk_join;

typedef struct dtk_engine_stats {
  uint64_t steps, tokens_out, joins, resumed, steps_below_half_occupancy, host_bound_steps, reader_wakeups, wasted_slot_steps;
  double   wait_s;               /* inside the device's wait: the step time the host sees                                           */
  double   launch_s, join_s;     /* inside launch / inside join execution (prefills, forks)                                         */
  double   idle_s;               /* sequences running but no step in flight (joins being executed, start-up)                        */
  double   drain_s;              /* waiting for steps in flight because a join / leave was queued                                    */
  double   first_launch_t, last_collect_t;   /* CLOCK_MONOTONIC seconds (0 = none yet)                                              */
} dtk_engine_stats;

int  dtk_engine_create(dtk_ctx* ctx, dtk_engine** out);
int  dtk_engine_create_ops(const dtk_engine_ops* ops, dtk_engine** out);
void dtk_engine_destroy(dtk_engine* e);            /* stops the loop (steps in flight are collected); readers see DTK_SEQ_LEFT     */
const char* dtk_engine_last_error(const dtk_engine* e);   /* text of the device failure that stopped the loop ("" = none)          */
/* tokens that end a reader's burst (the newline table of DetikzifyGenerator.rollout, reference infer/generate.py:262-274) */
int  dtk_engine_set_flush_tokens(dtk_engine* e, const int64_t* ids, int n);
/* option "depth" = steps kept in flight (1 | 2, default 2); "drain" (value ignored) = return once no step is in flight — the loop
 * collects the last steps behind sequences that have left on its own; meant for an engine none of whose sequences is decoding */
int  dtk_engine_set_option(dtk_engine* e, const char* name, int value);
/* n sequences are about to join: no step before all of them have, or timeout_ms have passed (rollouts started together move together) */
int  dtk_engine_expect(dtk_engine* e, int n, int timeout_ms);
/* queue a sequence and block until the loop has put its prompt into the slot (DTK_OK) or failed to (error_out).  Joins execute in
 * the order they were queued; dtk_engine_submit queues without waiting (a caller that plans joins against its own bookkeeping —
 * which slot holds which image prefix — queues under the lock that protects the bookkeeping and waits outside it);
 * dtk_engine_await blocks for that join's result.  `j` must stay valid until await returns; every ticket must be awaited once. */
int  dtk_engine_join(dtk_engine* e, dtk_join* j);
int  dtk_engine_submit(dtk_engine* e, dtk_join* j, uint64_t* ticket_out);
int  dtk_engine_await(dtk_engine* e, uint64_t ticket);
/* block until slot's sequence has undelivered flushed tokens, has ended, or timeout_ms passed (< 0: no timeout); copies up to cap
 * tokens; *state_out = DTK_SEQ_*.  A sequence that ended hands out its remaining tokens first: FINISHED / LEFT is reported
 * together with the last of them.  A device failure returns its error code (text: dtk_engine_last_error). */
int  dtk_engine_read(dtk_engine* e, int slot, int64_t* tokens_out, int cap, int32_t* n_out, int32_t* state_out, int timeout_ms);
/* end slot's sequence now (its undelivered tokens stay readable); the slot can be joined again at once */
int  dtk_engine_leave(dtk_engine* e, int slot);
int  dtk_engine_get_stats(dtk_engine* e, dtk_engine_stats* out);
/* ABI 7, additive: text-conditioned sequences (the TikZero adapter) in the engine's slots.  dtk_engine_submit_text queues a join like
 * dtk_engine_submit whose tower is conditioned on text_ids (1 <= n_text, no padding; caller-owned until the join is awaited, as
 * `ids` and `pixels`); pixels == NULL means the adapter's dummy input, as in dtk_prefill_slot_text.  Every prefill of such a join
 * (prefix encode, in-place reuse, fork tail, full) is the text prefill, and resume / prefix-cache checks compare the slot's cache under
 * the pair key dtk_text_image_key(image_key, text_key): the same pixels under another text, or under none, never share a slot's
 * prefix.  dtk_engine_set_prefill_text_op gives an engine of dtk_engine_create_ops the device's text prefill (dtk_engine_create wires
 * dtk_prefill_slot_text itself); a text join on an engine without it fails in submit with DTK_ERR_STATE (error_out says why).
 * Every join that forks a whole prefix-cache slot first checks (slot_lcp under its key) that the slot still holds the prefix and
 * encodes it again if not. */
int  dtk_engine_submit_text(dtk_engine* e, dtk_join* j, const int64_t* text_ids, int n_text, uint64_t text_key, uint64_t* ticket_out);
int  dtk_engine_set_prefill_text_op(dtk_engine* e, int (*prefill_slot_text)(void* dev, int slot, const int64_t* ids, int T, const float* pixels,
                                                                         uint64_t image_key, const int64_t* text_ids, int n_text,
                                                                         uint64_t text_key, int flags));

/* Tuning aids (tools/, bench): time one decode GEMV role (0 qkv, 1 o_proj, 2 gate/up, 3 down,
 * 4 lm_head; 5 / 6 = the batched gate/up kernel / its LDS-DMA twin with parts switched off, tools/probe_batch.py) in kernel
 * variant `variant` over all layers with HIP events (clobbers the decode state); select the variant the decode step uses for a
 * role: epi 1 = residual roles (down, and o_proj unless slot 5 is set), 2 qkv, 3 gate/up, 4 lm_head, 5 = o_proj alone (-1: as
 * epi 1), 6 = o_proj with the attention-partials prologue.  Variant 0 = the measured default of the model's width;
 * dtk_bench_gemv variant 0xff = whatever the decode step itself launches for that role (bench.py's roofline leg); 0xff | 0x800 =
 * the same on the context's weight format (fp8 rows, MXFP4 codes; without the bit the bf16 tensors are streamed); 0x800 with any
 * other variant or with the plain-probe bits fails with DTK_ERR_ARG.  In a bf16 context with option "w13" = 1, 0xff streams what the
 * step streams: the 13-bit planes of the roles that have them, in the step's shape (dtk_stats.probe_kernel_bytes describes role 2 of
 * that); 0x2000 | 0xff = the bf16 rows in the step's bf16 kernel whatever "w13" says, so one process can time both; 0x1000 | shape
 * (no other flag) = the role's planes in that 13-bit shape - o_proj, whose matrices the step keeps as bf16 rows, is packed for the
 * call alone; DTK_ERR_STATE for a role without planes (an unpackable row, a bf16 fold order no 13-bit shape has). */
int  dtk_bench_gemv(dtk_ctx* ctx, int role, int variant, int reps, float* avg_us);
int  dtk_set_gemv_variant(dtk_ctx* ctx, int epi, int variant);
/* Tuning switches; every default is the measured-best setting.  Single-sequence decode: "attn_threads" (0 =
 * contiguous key range per split | 256 | 512 | 1024 = tile-interleaved splits), "attn_splits" (1..16), "attn_combine" (0 = the
 * split partials are reduced in o_proj's prologue, 1 = by the last-arriving split block, 2 = by an own kernel),
 * "attn_full_max" (contexts below it use the one-block-per-head kernel), "w13" (bf16 contexts: 1 = stream the 13-bit planes of the
 * weight rows, packed lazily from the bf16 tensors, bit-identical results; 0 = the bf16 rows; drops the captured step; refused while
 * single-sequence steps are unread).  Batched decode: "tail_threads" (64 | 128 | 256 | 512) and "prefix_mfma" (1: the prefix a group of <= 16 forked slots
 * shares — same source slot, same length — is scored once for the group on the matrix cores by k_attn_prefix_g, the slots' private
 * keys per slot; 0 = every slot walks its whole context) default by the CONTEXT's size: 128 / 1 with 64 decoding slots, 256 / 0 below;
 * "pfx_splits" (1..4 key splits of that kernel, default 4), "gemv_bus" (64-slot qkv / gate-up by k_gemv_bus — a block per CU whose 8
 * waves are the 8 K slices, every operand straight from memory into the wave's registers, the slice sums met in LDS once: 0 off, 128 = the measured
 * default per role and weight format, else bit 0 qkv, bit 1 gate/up), "gemv_bc" (64-slot qkv / gate-up / lm_head by k_gemv_bc — a compute wave per 16-slot
 * column tile, x from L2 into registers, the weights through an LDS ring: 0 off, 128 = the measured default per role and weight format, else bit 0 qkv, bit 1
 * gate/up, bit 2 lm_head, bits 4..6 units per block), "gemv_b_wide" (0..6: row tiles per block), "gemm_b" (0 = x fragments in
 * registers, 1..4 = x through LDS by LDS-DMA), "gemv_bx" (0 off, 1 = x once per CU for gate/up + lm_head at 49..64 slots, 2..4 =
 * forced units per block), "gemv_bk" (K split across CUs for o_proj / down; slower, off), "gqa_fused" (GQA models: 0 = an attention block per query
 * head, 1 = per K/V head, 2 = per pair of query heads), "share_prefix_reads", "resid_split" (o_proj / down: two row tiles x half of
 * the slots per block), "resid_kparts" (o_proj / down at 49..64 slots: K-slice partials stored, reduced by the RMSNorm kernel that
 * follows), "gemv_bkl" (that kernel with LDS-DMA operand rings), "gemv_bl" (bit 0: loader-wave kernel for gate/up + lm_head, bit 1:
 * qkv by pair units, bit 2: fp8 weights too, bit 3 / 4: qkv as a RoPE pair unit + a V row tile per block, bit 5: fp8 weights at K = 4096 through registers), "gemv_xw" (x fragments
 * by an extra wave's ordinary loads instead of LDS-DMA), "attn_nt" (non-temporal K / V loads), "mv_slots" (0..4: contexts with at most
 * that many + 1 slots decode with the multi-vector kernels; 0 = the MFMA kernels for every context), "mv_tail_threads" (256 | 512 |
 * 1024: attention block of that step), "mv_shape_qkv|o|gu|down|lm_head" (-1 = measured default, 0 = the single-sequence block
 * shape, 1..3 = persistent with 8 / 4 / 16 waves).  Prefill / ViT: "attn_impl" (0 auto,
 * 1 VALU, 2 MFMA flash), "gemm_tile" (0 auto, 1 64x64, 2 128x64, 3 128x128, 4 64x32, 5 32x32), "gemm_bk" (64 | 128), "gemm_stages"
 * (1..4), "gemm_impl" (0 register-staged, 1 LDS-DMA fragment order, 2 128x128 LDS-DMA row order, 3 auto), "gemm_ring" (2..4),
 * "gemm_glds_min_tiles".  fp8 models: "act_fp8" (0 = default: bf16 activations, the fp8 weights widened in registers; 1 = OPT-IN: the MFMA-family
 * step runs on the fp8 matrix cores with MXFP8 activations — 15-26 % shorter steps, logits ~0.12 rel-L2 from the bf16-activation step:
 * tests/test_gpu_parity_batched.py::test_mxfp8_activations_against_bf16_activations asserts <= 0.20), "mx_nc_qkv" / "mx_nc_gu" / "mx_nc_lm_head" (0..4 compute waves per block of its unit kernel; 0 = from the CU count).
 * DESIGN.md 3.4 has the defaults and what each switch measured.
 * Diagnostic: "vit_feature_layer" (0..depth-1) = the block whose normed output dtk_vit_encode returns as features (tests walk
 * the tower block by block with it); every cached image prefix is dropped.
 * Decoder prefill: "prefill_sk" (1 = roles sliced along K by their weight shape, the default; 0 = one-chain GEMMs — another fp32
 * summation order, cached prefixes are dropped; 2 / 4 / 8 = a cap on the slices), and three bit-identical choices: "gemm_wt" (k_gemm_g3's W stage from the
 * fragment-major weight copy), "gemm_epi_direct" (k_gemm_g3 stores from the accumulator layout instead of through LDS), "qkv_rope_fused" (the
 * sliced q/k/v role reduces inside the RoPE + KV-append kernel), "swiglu_fused" (SiLU*mul is the epilogue of the gate/up GEMM), "gemm_sk_tile" (0 = 256 x 128, 1 = 128 x 256, 2 = by M), "gemm_g3_tile" (the one-chain k_gemm_g3: 0 = by shape, 1 = 256 x 128, 2 = 128 x 256).  "sk_sl_min_rows": above this many prefill rows a sliced role is ONE launch that folds
 * its slices in registers (k_gemm_g3<.., SL>) instead of (tile, slice) blocks + reduction per 512 rows; bit-identical.
 * The environment variable DTK_OPTIONS="name=value,name=value" applies the same switches at dtk_create.
 * SCOPE: the switches that select a kernel VARIANT ("gemv_*", "resid_*", "gemm_*", "mx_*", "attn_impl") are process-wide — they live in the
 * launchers, not in the context: a later context of the same process inherits what an earlier one set, and an A/B inside one process must set
 * the switch on both sides.  The per-context ones: "act_fp8", "prefix_mfma", "tail_threads", "pfx_splits", "share_prefix_reads", "mv_slots",
 * "attn_threads" / "attn_splits" / "attn_combine", "vit_feature_layer", "gemm_naive", "resid_kparts", "prefill_sk", "qkv_rope_fused", "swiglu_fused",
 * "logprobs" (0 | 1, see "Log-probabilities of sampled tokens" below). */
int  dtk_set_option(dtk_ctx* ctx, const char* name, int value);

/* Op-level entry points used by the parity tests (tests/): run ONE kernel of the
 * hot path on host buffers.  All matrices row-major; bf16 as uint16.  They exist so a
 * failing kernel can be isolated on the GPU box; the product path never calls them. */
#define DTK_EPI_NONE 0
#define DTK_EPI_BIAS 1        /* + bias[n]                         */
#define DTK_EPI_GELU 2        /* gelu(acc + bias)                   */
#define DTK_EPI_RESIDUAL 4    /* bf16(acc + bias) + residual[m,n]   */
#define DTK_GEMM_NAIVE 256    /* use the non-MFMA reference kernel  */
#define DTK_GEMM_WT 512       /* also hand the kernel W as fragment-major tiles (what the decoder prefill does): same result, bit for bit */
#define DTK_GEMM_SL 1024      /* with K slices: ONE launch that folds the slices in registers (what large M takes) instead of (tile, slice) blocks + reduction */
#define DTK_GEMM_KSLICES_SHIFT 12   /* flags |= S << 12 (S = 1..8): the sliced-K family of the decoder prefill — K's 64-wide k-tiles cut into S
                                     * runs, a chain per run, the runs' sums added in order (fp32); either kernel (MFMA / naive) */
/* C[M,N] = A[M,K] . W[N,K]^T (+epilogue) */
int  dtk_op_gemm(dtk_ctx* ctx, const uint16_t* A, const uint16_t* W, const uint16_t* bias,
                 const uint16_t* residual, int M, int N, int K, int flags, uint16_t* C);
/* C = residual + bf16(bf16(sigmoid(gate)) * bf16(A . W^T + bias)) (the adapter's gated residuals, GEMM_GATED_RESIDUAL); gate = one bf16;
 * flags: DTK_GEMM_NAIVE only; the kernel is whatever the tuning switches ("gemm_impl", "gemm_tile", ...) select for the shape */
int  dtk_op_gemm_gated(dtk_ctx* ctx, const uint16_t* A, const uint16_t* W, const uint16_t* bias, const uint16_t* residual,
                       const uint16_t* gate, int M, int N, int K, int flags, uint16_t* C);
/* the scoring kernel pair alone: Xn [M][K] = final-normed hidden rows, W [N][K] = lm_head, targets [M] in [0, N).  Per row:
 * logprob = z[target] - logsumexp(z), lse, argmax (lowest index on ties), zmax = z[argmax], z = bf16-rounded Xn . W^T.
 * flags: DTK_GEMM_WT only.  lse_out / argmax_out / zmax_out may be NULL.  The op's scratch (the records included) starts as 0xFF bytes
 * and the 256 guard bytes behind every result must still hold them (DTK_ERR_STATE).  dtk_gemm_last_kernel() afterwards: family 7, tile
 * 6 / 7 (k_gemm_g3<LS> 256x128 / 128x256, + WT << 13) or 3 (k_gemm_mfma<64, 128, LS>). */
int  dtk_op_score(dtk_ctx* ctx, const uint16_t* Xn, const uint16_t* W, const int32_t* targets, int M, int N, int K, int flags,
                  float* logprob_out, float* lse_out, int32_t* argmax_out, float* zmax_out);
/* mode 0: y = W.x ; mode 1: y = W.rmsnorm(x, norm_w) ; fp32 result of the bf16-rounded output */
int  dtk_op_gemv(dtk_ctx* ctx, const uint16_t* W, const uint16_t* x, const uint16_t* norm_w,
                 int N, int K, int mode, float eps, uint16_t* y);
/* dtk_op_gemv on MXFP4 weights: W [N][K] row-major bf16 is quantised by the loader's own quantiser (blocks of 32 along K, the last one
 * of a row may be ragged) and streamed by the decode kernel; y [N] as dtk_op_gemv; w_eff_out (or NULL) [N][K] = the de-quantised weights */
int  dtk_op_gemv_q4(dtk_ctx* ctx, const uint16_t* W, const uint16_t* x, const uint16_t* norm_w,
                    int N, int K, int mode, float eps, uint16_t* y, uint16_t* w_eff_out);
/* the multi-vector GEMV of the <= 4-slot step on nb (1, 2, 4) row-major vectors X[nb][K] -> Y[nb][N]; per vector bit-identical
 * to dtk_op_gemv */
int  dtk_op_gemv_mv(dtk_ctx* ctx, const uint16_t* W, const uint16_t* X, const uint16_t* norm_w,
                    int N, int K, int mode, float eps, int nb, uint16_t* Y);
/* The fp8 matrix-core GEMVs of the batched step of an fp8 model (csrc/kernels_batch_mx.hip; BASELINE config 5's "CDNA4 fp8 MFMA"):
 * W8 [N][K] e4m3 bytes + wscale [N] (per-row power of two); X [nslots][K] bf16 rows, quantised to MXFP8 in groups of G = 32 | 16
 * consecutive k by the step's own quantiser; nslots = 16 | 32 | 64.  mode 0: unit kernel with the logits epilogue (G = 32):
 * Y [nslots][N] = bf16-rounded sums; mode 1: the K-slice kernel of the N = d roles: Y = the 8 slice partials added in order (fp32);
 * mode 2: unit kernel with the SwiGLU epilogue (N = 2 ff): y8_out / ys_out = the activation as MXFP8 groups of 16 (64 ff bytes /
 * ceil(ff / 256) KiB).  x8_out (64 K bytes) / xs_out (ceil(K / (16 G)) KiB), optional: the quantised input in the kernels' order. */
/* byte offsets of value k of `slot` and of its group's E8M0 scale in the MXFP8 activation buffers (G = 32 | 16); host arithmetic only */
int  dtk_mx_layout(int G, int slot, int k, int64_t* data_off, int64_t* scale_off);
int  dtk_op_gemv_mx(dtk_ctx* ctx, const uint8_t* W8, const float* wscale, const uint16_t* X, int N, int K, int G, int nslots, int mode,
                    float* Y, uint8_t* x8_out, uint8_t* xs_out, uint8_t* y8_out, uint8_t* ys_out);
/* softmax(Q K^T * scale [+ causal mask with q_offset]) V, heads-major [H][T][hd] bf16 */
int  dtk_op_attention(dtk_ctx* ctx, const uint16_t* Q, const uint16_t* K, const uint16_t* V,
                      int H, int Tq, int Tk, int hd, int causal, int q_offset, uint16_t* O);
/* the segmented causal attention of dtk_score_packed alone (hd 128 | 64, the MFMA kernel): Tk keys of which the first shared_len are
 * visible to every query; query t sees key j iff j <= kv_row[t] and (j < shared_len or j >= seg_begin[t]); 0 <= seg_begin[t] <= kv_row[t] < Tk */
int  dtk_op_attention_seg(dtk_ctx* ctx, const uint16_t* Q, const uint16_t* K, const uint16_t* V,
                          int H, int Tq, int Tk, int hd, int shared_len, const int32_t* seg_begin, const int32_t* kv_row, uint16_t* O);
/* Decode attention alone, op by op (additive, ABI 7); bf16 bits throughout, scale = hd^-0.5.
 * dtk_op_attn_decode: the single-sequence kernels.  q [H*hd], K / V [KVH][T_max][hd] (query head h reads K/V head h / (H / KVH)), hd 128 | 64.
 * The caches are uploaded once; for each of the npos positions the step's launcher runs over keys 0..pos[i] and out[i][H*hd] receives
 * the head outputs.  threads 0 (contiguous key ranges per split, hd 128 only) | 256 | 512 | 1024 (tiles dealt round-robin), splits 1..16,
 * mode 2 = own combine kernel, 1 = in-kernel combine (threads 0; fails with DTK_ERR_STATE unless the arrival counters are zero again),
 * 3 = one block per head (threads 0), 0 = consumer-side combine: o_proj's prologue reduces the partials, run with an identity weight
 * onto a zero residual (variant -1 = the step's default kernel, 0..8 = that tuning variant); mode 0 also returns the raw partials
 * pm_out / pl_out [npos][H][splits] and po_out [npos][H][splits][hd] (NaN where none are written: threads != 0 with one split).
 * pm_out / pl_out / po_out may be NULL in the other modes. */
int  dtk_op_attn_decode(dtk_ctx* ctx, const uint16_t* q, const uint16_t* K, const uint16_t* V, int H, int KVH, int hd, int T_max,
                        const int32_t* pos, int npos, int threads, int splits, int mode, int variant, uint16_t* out,
                        float* pm_out, float* pl_out, float* po_out);
/* dtk_op_attn_decode_b: the batched kernels (head dim 128, bf16 output).  nslots = the grid's slot dimension: 1 | 2 | 4 (the multi-vector
 * step: use_prefix 0, tail_threads up to 1024) | 16 | 32 | 64; q [nslots][H*128], K / V [nslots][KVH][T_max][128]; per slot pos, active,
 * share_src (-1 = none; else rows [0, share_len) are read from that slot's cache, share_len <= pos) and share_len.  use_prefix = score
 * the shared prefixes per group on the matrix cores (the groups are formed as dtk_decode_batch_launch forms them), pfx_splits 1..4,
 * tail_threads 64 | 128 | 256 | 512 (| 1024), gqa_fused 0..2, attn_nt 0 | 1: the options of the same names.  out [nslots][H*128] row-major;
 * every element is set to 0xFFFF first, which the rows of inactive slots keep. */
int  dtk_op_attn_decode_b(dtk_ctx* ctx, const uint16_t* q, const uint16_t* K, const uint16_t* V, int nslots, int H, int KVH, int T_max,
                          const int32_t* pos, const int32_t* active, const int32_t* share_src, const int32_t* share_len,
                          int use_prefix, int pfx_splits, int tail_threads, int gqa_fused, int attn_nt, uint16_t* out);
/* dtk_op_attn_decode_b8 (additive, ABI 7): the same launch through the instantiations of a kv_format-mxfp8 context.  kv8_from[nslots]
 * (share_len <= kv8_from <= pos for active slots) and the four shadow planes, IN/OUT host arrays: codes [nslots][KVH][T_max][128] and
 * E8M0 scales [nslots][KVH][T_max][4] for K and for V.  Rows [kv8_from, pos) of an active slot are read from them (code * 2^(scale - 127));
 * row pos is read in bf16, quantised, scored de-quantised, and its codes and scales are stored — by exactly one block per (slot, kv head).
 * Nothing else of the planes is written: they come back as they went in but for those rows.  After the launch the op reads the bf16 K
 * and V back and compares them with the caller's arrays: a changed byte fails the call with DTK_ERR_STATE (the first element is named). */
int  dtk_op_attn_decode_b8(dtk_ctx* ctx, const uint16_t* q, const uint16_t* K, const uint16_t* V, int nslots, int H, int KVH, int T_max,
                           const int32_t* pos, const int32_t* active, const int32_t* share_src, const int32_t* share_len,
                           const int32_t* kv8_from, uint8_t* k8_codes, uint8_t* k8_scales, uint8_t* v8_codes, uint8_t* v8_scales,
                           int use_prefix, int pfx_splits, int tail_threads, int gqa_fused, int attn_nt, uint16_t* out);
/* The weight kernels of the batched (<= 64 slot) decode step alone, op by op (additive, ABI 7); bf16 bits throughout.
 * dtk_op_gemv_b: one role through the step's dispatcher; the process-wide options ("gemv_bx", "gemv_bl", "gemv_bc", "gemv_bus",
 * "gemv_b_wide", "resid_split", "gemv_br_wd", "gemv_loaders", "gemv_xw") choose the kernel as they do in the step.  epi: 0 STORE,
 * 1 RESID, 2 QKV, 3 SWIGLU, 4 LOGITS.  Weights: W [N][K] bf16, or W8 [N][K] e4m3 bytes + wscale [N] (per-row power of two) — exactly
 * one of the two; they are tiled on the device by the loader's kernels.  X [nslots][K]; with norm_w [K] (+ eps) X is a residual stream
 * and the step's RMSNorm kernel produces the GEMV input (xn_out [nslots][K], optional: those rows; idle slots' rows are 0), without
 * it X is the input itself.  active [nslots], pos [nslots] (QKV; 0 <= pos < T_max for active slots); slots >= nslots are idle; the
 * column-tile count follows from nslots as in dtk_decode_batch_launch (1: <= 16, 2: <= 32, else 4).  K % 8 == 0.
 * Every result buffer is IN/OUT and sized for all 64 slots, so that a caller can pre-fill it and see what was written:
 *   QKV (N = (H + 2 KVH) * 128, d = H * 128, rope_cos / rope_sin [T_max][64]): q_io [64][d], k_io / v_io [64][KVH][T_max][128];
 *   RESID (y += bf16(W.x)) / STORE: y_io [64][N];   LOGITS: logits_io [64][N] fp32;
 *   SWIGLU (N = 2 ff, ff % 8 == 0 as in dtk_create, rows = gate rows then up rows): frag_io = the raw fragment-major activation buffer, 4 * ceil(ff / 32) * 512
 *   elements (slot s, row i at ((s / 16 * ceil(ff / 32) + i / 32) * 64 + i % 32 / 8 * 16 + s % 16) * 8 + i % 8), and y_io
 *   [nslots][ff] (out only) = the same values row-major.
 * Buffers a role does not use may be NULL.  err_out = the launch's count of expired in-kernel hand-off waits (0 unless a kernel hung). */
int  dtk_op_gemv_b(dtk_ctx* ctx, int epi, const uint16_t* W, const uint8_t* W8, const float* wscale, int N, int K,
                   const uint16_t* X, const uint16_t* norm_w, float eps, const int32_t* active, const int32_t* pos, int nslots,
                   int d, int ff, int H, int KVH, int T_max, const uint16_t* rope_cos, const uint16_t* rope_sin,
                   uint16_t* q_io, uint16_t* k_io, uint16_t* v_io, uint16_t* y_io, uint16_t* frag_io, float* logits_io,
                   uint16_t* xn_out, uint32_t* err_out);
/* dtk_op_gemv_bkp: the N = d roles of the 33..64-slot step as its two launches — the K-slice weight kernel ("gemv_bkl" 0: k_gemv_bkp,
 * 1: k_gemv_bkl, with "gemv_xw" x waves), then k_resid_norm_b with norm_w [N].  resid_io [64][N]: the residual streams, updated in place
 * for the active slots; xn_io [64][N]: the normalised rows (row-major here, fragment-major on the device); part_out [8][64][N] fp32:
 * the eight K-slice partials (written for all 64 columns).  DTK_ERR_ARG, with nothing launched and no buffer touched, for a shape the
 * step itself would not give to these kernels (fewer than 33 slots, N other than 2048 / 4096, a K that leaves one of the 8 slices
 * empty, fp8 weights with "gemv_bkl" 0). */
int  dtk_op_gemv_bkp(dtk_ctx* ctx, const uint16_t* W, const uint8_t* W8, const float* wscale, int N, int K, const uint16_t* X,
                     const int32_t* active, int nslots, const uint16_t* norm_w, float eps, uint16_t* resid_io, uint16_t* xn_io,
                     float* part_out, uint32_t* err_out);
/* The single-sequence decode GEMV family alone, one role at a time (additive, ABI 7); bf16 bits throughout.  pro: 0 COPY (x [K] is the
 * input), 1 RMSNORM (x is a residual stream, norm_w [K], eps), 2 ATTN (the input is the combine of S = 1..16 split-K attention partials
 * pm / pl [H][S], po [H][S][hd], K = H * hd).  epi: 0 STORE, 1 RESID, 2 QKV, 3 SWIGLU, 4 LOGITS.  Weights, exactly one of: W [N][K] bf16;
 * W8 [N][K] e4m3 bytes + wscale [N] (per-row power of two; K % 16 == 0); W4 [N][ceil(K/32)*16] E2M1 codes + S4 [N][ceil(K/32)] E8M0 block
 * scales (MXFP4: byte i of a row = weights 2i low nibble, 2i + 1 high nibble, rows padded with zero codes to whole blocks of 32).
 * variant: bf16 -1 = the step's choice for hidden size d, else a row of the tuning table; fp8 -1 = the process default
 * (DTK_F8_VARIANT), 0..9 = that shape; MXFP4 -1 only.  K % 8 == 0, hd 128 | 64, ff % 8 == 0 as in dtk_create.
 * Result buffers are IN/OUT, so that a caller can pre-fill them and see what was written:
 *   QKV (N = (H + 2 KVH) * hd, d = H * hd, H % KVH == 0, rope_cos / rope_sin [T_max][hd / 2], 0 <= pos < T_max): q_io [H * hd],
 *   k_io / v_io [KVH][T_max][hd] (row pos of every head is written);   STORE: y_io [N];   RESID: y_io [N] += bf16(W . x);
 *   SWIGLU (N = 2 ff, rows = gate rows then up rows): y_io [ff];   LOGITS: logits_io [N] fp32.
 * scratch_fill: the byte the op's device scratch is filled with before the operands are uploaded (what a kernel reads beside them).
 * DTK_ERR_ARG, with nothing launched and no buffer touched, for a shape or a (pro, epi, format, variant) the step would never run.
 * DTK_ERR_STATE if the launch wrote behind the end of a result buffer (256 guard bytes each).  Buffers a role does not use may be NULL. */
int  dtk_op_gemv_role(dtk_ctx* ctx, int pro, int epi, int variant, const uint16_t* W, const uint8_t* W8, const float* wscale,
                      const uint8_t* W4, const uint8_t* S4, int N, int K, int d, int ff, int H, int KVH, int hd, int T_max, int pos, float eps,
                      const uint16_t* x, const uint16_t* norm_w, const uint16_t* rope_cos, const uint16_t* rope_sin,
                      int S, const float* pm, const float* pl, const float* po, int scratch_fill,
                      uint16_t* q_io, uint16_t* k_io, uint16_t* v_io, uint16_t* y_io, float* logits_io);
/* The prefill's row kernels and attention layouts alone (additive, ABI 7); bf16 bits throughout, every operand from the host.  As in
 * dtk_op_gemv_role the result buffers (*_io) are IN/OUT, scratch_fill is the byte the op's device scratch holds around the operands, a
 * write behind the end of a result buffer (256 guard bytes each) is DTK_ERR_STATE, and what the prefill would never hand a kernel is
 * DTK_ERR_ARG with nothing launched and no buffer touched.
 * dtk_op_rope_scatter: form 0 = launch_rope_scatter on QKV [T][(H + 2 KVH) hd]; form 1 = launch_sk_rope_scatter on fp32 partials
 *   part [S][part_rows][(H + 2 KVH) hd] (S = 1..8, part_rows >= T).  rows = NULL: row t at position and cache row start_pos + t; else
 *   rows [T][2] = {position, cache row} (the _rows launchers).  rope_cos / rope_sin [max_pos][hd / 2].  q_io [H][T][hd], k_io / v_io
 *   [KVH][T_max][hd].  hd 128 | 64, H % KVH == 0, positions < max_pos, cache rows < T_max.
 * dtk_op_rows_norm: form 0 launch_rmsnorm_rows, 1 launch_rmsnorm_rows_sk, 3 launch_layernorm_rows (norm_w, ln_b; X = NULL: in place on
 *   y_io, ldx = ldy): X [M][ldx] -> y_io [M][ldy], N = the row length (N % 8 for forms 0 / 3, N % 4 for form 1).  form 2 = launch_sk_reduce
 *   on part [S][part_rows][N] (N % 4 == 0): flags DTK_EPI_BIAS | DTK_EPI_RESIDUAL | DTK_EPI_GATED_RESIDUAL with bias [N], residual [M][ldr],
 *   gate [1]; c_io [M][ldc]; norm_w [N] (optional) -> y_io [M][ldy], the fused RMSNorm.
 * dtk_op_swiglu: form 0 launch_silu_mul on GU [M][2 ff] (ldact == ff); form 1 launch_sk_reduce_swiglu on part [S][part_rows][2 ff]
 *   (ff % 4 == 0); form 2 A [M][K], W [2 ff][K] (gate rows, then up rows): launch_retile_pairs + launch_gemm_g3_swiglu, DTK_ERR_ARG where
 *   that launcher declines (see "gemm_g3_min_blocks").  act_io [M][ldact].
 * dtk_op_attention_ex: launch_attention on raw buffers of nq / nk / nv / no elements; strides [12] = {q_sh, q_st, q_sb, k_sh, k_st, k_sb,
 *   v_sh, v_st, v_sb, o_sh, o_st, o_sb} (head, token, batch; elements).  Query head h reads K / V head h / kv_group.  Strides that address
 *   outside a buffer are refused, and under "attn_impl" 2 so are operands the MFMA kernel does not take (no silent VALU fallback).
 * dtk_op_rows_move: form 0 launch_embed_gather (ids [M] in [0, V), src = table [V][D]) -> dst_io [M][D]; form 1 launch_copy_rows
 *   src [M][lds] -> dst_io [M][ldd]; form 2 launch_im2col pixels fp32 [3][image][image] -> dst_io [(image / patch)^2][ldd]. */
#define DTK_EPI_GATED_RESIDUAL 8   /* dtk_op_rows_norm form 2, with DTK_EPI_RESIDUAL: residual + bf16(bf16(sigmoid(gate)) * bf16(sum + bias)) */
int  dtk_op_rope_scatter(dtk_ctx* ctx, int form, const uint16_t* QKV, const float* part, int S, int part_rows, int T, int H, int KVH, int hd,
                         int T_max, int start_pos, const int32_t* rows, int max_pos, const uint16_t* rope_cos, const uint16_t* rope_sin,
                         int scratch_fill, uint16_t* q_io, uint16_t* k_io, uint16_t* v_io);
int  dtk_op_rows_norm(dtk_ctx* ctx, int form, const uint16_t* X, const float* part, int S, int part_rows, const uint16_t* norm_w,
                      const uint16_t* ln_b, const uint16_t* bias, const uint16_t* residual, const uint16_t* gate, int flags, int M, int N,
                      int ldx, int ldc, int ldr, int ldy, float eps, int scratch_fill, uint16_t* c_io, uint16_t* y_io);
int  dtk_op_swiglu(dtk_ctx* ctx, int form, const uint16_t* GU, const float* part, int S, int part_rows, const uint16_t* A, const uint16_t* W,
                   int M, int ff, int K, int ldact, int scratch_fill, uint16_t* act_io);
int  dtk_op_attention_ex(dtk_ctx* ctx, const uint16_t* Q, int64_t nq, const uint16_t* K, int64_t nk, const uint16_t* V, int64_t nv,
                         uint16_t* o_io, int64_t no, const int64_t* strides, int H, int kv_group, int Tq, int Tk, int hd, int causal,
                         int q_offset, int nbatch, int scratch_fill);
int  dtk_op_rows_move(dtk_ctx* ctx, int form, const int32_t* ids, const uint16_t* src, const float* pixels, int M, int D, int V, int lds,
                      int ldd, int image, int patch, int scratch_fill, uint16_t* dst_io);
/* The prefill GEMM family alone, as the product calls it (additive, ABI 7): ONE call of launch_gemm_mfma (default), launch_gemm_naive
 * (DTK_GEMM_NAIVE), launch_gemm_sk (S << DTK_GEMM_KSLICES_SHIFT) or launch_gemm_g3_sliced (+ DTK_GEMM_SL) on host operands.  A [.. na], W [.. nw],
 * bias [.. nb], residual [.. nr] and c_io [.. nc] are whole buffers of that many elements; row m of A starts at m * lda, row n of W at n * ldw, and
 * the first used element of bias / residual / C lies b_off / r_off / c_off elements inside its buffer (every buffer is uploaded 256-byte aligned,
 * so an offset of 1, 2 or 4 elements gives the kernel a pointer that is 2-, 4- or 8-byte aligned only); rows of residual / C are ldr / ldc apart.
 * flags: DTK_EPI_BIAS, DTK_EPI_GELU (the context's GELU) or DTK_EPI_GELU_ERF / DTK_EPI_GELU_TANH (that GELU whatever the context's config),
 * DTK_EPI_RESIDUAL, DTK_EPI_GATED_RESIDUAL (with DTK_EPI_RESIDUAL; gate = one bf16), DTK_GEMM_INPLACE (with DTK_EPI_RESIDUAL: residual = NULL,
 * c_io holds the residual on entry, the kernel gets residual = C and ldr = ldc — every ViT and adapter block), DTK_GEMM_NAIVE, DTK_GEMM_WT,
 * DTK_GEMM_SL, S << DTK_GEMM_KSLICES_SHIFT.  c_io is IN/OUT (uploaded first): what the launch does not write keeps the caller's bits.
 * scratch_fill and the 256 guard bytes behind c_io (DTK_ERR_STATE) as in dtk_op_gemv_role.  DTK_ERR_ARG with nothing launched: lda / ldw not a
 * multiple of 8 or below K (A and W are 16-byte aligned rows in the product), strides or offsets that address past na / nw / nb / nr / nc (the
 * message names the operand), more than 8 slices, a shape the sliced kernels do not take (K < 128, N % 4).
 * *kernel_out (may be NULL) = the launchers' record of the kernel that ran: family | tile << 4 | stages << 8 | bk128 << 12 | WT << 13 |
 * epilogue << 14 | slices << 16 — family 1 k_gemm_mfma, 2 k_gemm_glds, 3 k_gemm_g3, 4 k_gemm_g3<SK> + k_sk_reduce, 5 k_gemm_g3<SL>, 6 k_gemm_naive
 * (7: the log-softmax epilogue behind dtk_op_score, see there); tile 1 = 64x64, 2 = 128x64, 3 = 128x128, 4 = 64x32, 5 = 32x32, 6 = 256x128, 7 = 128x256; epilogue (k_gemm_g3 forms) 1 = through LDS, 2 = direct.
 * dtk_gemm_last_kernel(): the same record after any GEMM launch of the process (dtk_op_gemm, dtk_op_gemm_gated, ...).
 * Option "gemm_g3_tile" (process-wide; bit-identical): the block tile of the one-chain k_gemm_g3 — 0 = by shape (default), 1 = 256 x 128,
 * 2 = 128 x 256 — as "gemm_sk_tile" for the sliced kernels. */
#define DTK_EPI_GELU_ERF 16    /* dtk_op_gemm_ex: gelu_erf(acc + bias), whatever the context's config */
#define DTK_EPI_GELU_TANH 32   /* dtk_op_gemm_ex: gelu_tanh(acc + bias) */
#define DTK_GEMM_INPLACE 64    /* dtk_op_gemm_ex: the residual is C itself */
int  dtk_op_gemm_ex(dtk_ctx* ctx, const uint16_t* A, int64_t na, const uint16_t* W, int64_t nw, const uint16_t* bias, int64_t nb,
                    const uint16_t* residual, int64_t nr, const uint16_t* gate, uint16_t* c_io, int64_t nc, int M, int N, int K,
                    int lda, int ldw, int ldr, int ldc, int b_off, int r_off, int c_off, int flags, int scratch_fill, int* kernel_out);
int  dtk_gemm_last_kernel(void);
/* The multi-vector decode GEMV family (the step of a context with at most 5 slots) alone, one role at a time (additive, ABI 7): one
 * (pro, epi) of launch_gemv_mv on host operands, nb = 1 | 2 | 4 slots, head dim 128.  pro / epi as in dtk_op_gemv_role; the pairs are the
 * step's (RMSNORM, QKV), (COPY, RESID), (RMSNORM, SWIGLU), (RMSNORM, LOGITS) and the tests' (COPY, STORE), (RMSNORM, STORE).  shape: -1 =
 * the step's measured choice (d tells o_proj, K == d, from down), 0..3 = that block shape; the choice holds for this call only.  Weights:
 * W [N][K] bf16, or W8 [N][K] e4m3 bytes + wscale [N] (K % 16 == 0).  pos [nb], active [nb] (0 = the slot is idle); bs_null != 0 hands the
 * kernel no BatchState at all (every slot must be active).  X: x_layout 0 = rows [nb][K]; 1 (PRO_COPY only) = the kernel's fragment order
 * as whole 16-slot tiles, ceil(K / 32) * 512 elements, value (slot, k) at ((k >> 5) * 64 + ((k & 31) >> 3) * 16 + slot) * 8 + (k & 7).
 * Result buffers are IN/OUT as in dtk_op_gemv_role: QKV (N = (H + 2 KVH) * 128, d = H * 128, H % KVH == 0, rope tables [T_max][64],
 * 0 <= pos[b] < T_max): q_io [nb][d], k_io / v_io [nb][KVH][T_max][128];   STORE / RESID: y_io [nb][N];   SWIGLU (N = 2 ff, ff % 8 == 0):
 * y_io = ceil(ff / 32) * 512 elements in fragment order;   LOGITS: logits_io [nb][N] fp32.  scratch_fill, the 256 guard bytes behind
 * every result buffer (DTK_ERR_STATE) and DTK_ERR_ARG with nothing uploaded or launched as in dtk_op_gemv_role; refused besides: an
 * LDS request (nb * K * 2 bytes of x plus the reduction words) beyond the CU's 160 KiB.  Buffers a role does not use may be NULL. */
int  dtk_op_gemv_mv_role(dtk_ctx* ctx, int pro, int epi, int nb, int shape, const uint16_t* W, const uint8_t* W8, const float* wscale,
                         int N, int K, int d, int ff, int H, int KVH, int T_max, const int32_t* pos, const int32_t* active, int bs_null,
                         int x_layout, const uint16_t* X, const uint16_t* norm_w, float eps, const uint16_t* rope_cos,
                         const uint16_t* rope_sin, int scratch_fill, uint16_t* q_io, uint16_t* k_io, uint16_t* v_io, uint16_t* y_io,
                         float* logits_io);
/* 13-bit planes of bf16 weight rows (csrc/w13.h; additive, ABI 7): the single-sequence step of a bf16 context streams them instead of the
 * 16-bit rows when dtk_set_option(ctx, "w13", 1); the kernels rebuild the rows' own bits, so every result is the bf16 step's.  A row
 * holding a weight more than 30 binades below its largest cannot be packed; its whole matrix then stays bf16 (dtk_stats.w13_counts).
 * dtk_op_gemv_role with bf16 operands and variant = 0x1000 + v packs W on the device and runs the role on the planes in 13-bit shape v
 * (0xff: the shape a step runs; DTK_ERR_ARG for a shape that does not exist); if a row is unpackable the bf16 kernel runs instead.
 * dtk_w13_op_bad_rows: the unpackable rows that call found (-1 before any).  dtk_w13_pack_host / dtk_w13_unpack_host: w13.h's host code
 * on rows [N][K] (K % 8 == 0), planes [N][dtk_w13_row_bytes(K)], hb [N]; bad[r] = weights of row r below its window (0: packed exactly;
 * otherwise the row must not be used).  No GPU needed. */
int  dtk_w13_row_bytes(int K);
int  dtk_w13_pack_host(const uint16_t* W, int N, int K, uint8_t* planes, uint8_t* hb, int32_t* bad);
int  dtk_w13_unpack_host(const uint8_t* planes, const uint8_t* hb, int N, int K, uint16_t* W);
int  dtk_w13_op_bad_rows(dtk_ctx* ctx);
/* The row byte the device keeps beside the planes is hb | 0x80 where a weight of the row has e >> 1 == 0 (w13.h: W13_ZROW): such rows
 * take the general decode, the others a shorter one with the same bits.  dtk_w13_row_bytes_host: that byte for rows [N][K] (no GPU).
 * dtk_w13_flagged_rows: rows with the bit among the packed matrices of role 0 q/k/v, 1 o_proj, 2 gate/up, 3 down, 4 lm_head (-1: no
 * planes yet).  Option "w13_nz" = 0 makes the packer set the bit in every row. */
int  dtk_w13_row_bytes_host(const uint16_t* W, int N, int K, uint8_t* bytes);
int  dtk_w13_flagged_rows(dtk_ctx* ctx, int role);
int  dtk_op_layernorm(dtk_ctx* ctx, const uint16_t* X, const uint16_t* w, const uint16_t* b,
                      int M, int D, float eps, uint16_t* Y);
/* run the sampler on host logits with the context's sampling config; step = draw index */
int  dtk_op_sample(dtk_ctx* ctx, const float* logits, int V, int step, int64_t* token_out,
                   float* filtered_probs_out);

/* Log-probabilities of sampled tokens (additive, ABI 7).  dtk_set_option(ctx, "logprobs", 1) (default 0; per context; a change of value is
 * refused with DTK_ERR_STATE while a batch step is in flight, while single-sequence steps are unread (dtk_set_sampling / dtk_prefill
 * start the sequence afresh) and while an engine of dtk_engine_create holds a sequence that has not left; it drops the captured decode graphs) makes every decode step deliver two fp32 values
 * with its token t, from the passes over the logits the sampler runs anyway:
 *   logprob        = z[t] - logsumexp(z) over the whole vocabulary, z = the fp32 row lm_head wrote (what dtk_prefill's logits_out
 *                    reads back): no temperature, no suppression list — the quantity dtk_score reports for the same position;
 *   sample_logprob = log(q[t] / total): the probability with which the sampler chose t, from its own integer masses
 *                    q = floor(exp(z' - z'max) * 2^31) over the kept set after suppression, temperature, top-k and top-p
 *                    (computed in double from the two integers); exactly 0 for a greedy step.
 * Both are NaN for a forced token (the first step of a dtk_resume_slot'ed slot) and for slots that took no part in the step.  With the
 * option off the steps run the same kernels and copies as before the option existed, and every *_lp call fails with DTK_ERR_ARG;
 * with it on the plain calls keep working (they drop the pairs).
 *   dtk_decode_wait_lp        dtk_decode_wait + lp_out[2] = (logprob, sample_logprob)
 *   dtk_decode_batch_wait_lp  dtk_decode_batch_wait + the two values per slot
 *   dtk_engine_read_lp        dtk_engine_read + the i-th pair of the i-th token returned.  The engine of dtk_engine_create collects the
 *                             pairs while its context's option is on (switch it before the first join) and fails with DTK_ERR_ARG
 *                             while it is off; an engine of dtk_engine_create_ops collects them through the op given to
 *                             dtk_engine_set_wait_lp_op (same contract as dtk_decode_batch_wait_lp; it then replaces ops.wait) and
 *                             delivers NaN pairs without one.
 *   dtk_op_sample_lp          dtk_op_sample + lp_out[2]; V may exceed the context's vocabulary (<= 262 144) when filtered_probs_out is NULL */
int  dtk_decode_wait_lp(dtk_ctx* ctx, int64_t* token_out, float* lp_out /* [2] */);
int  dtk_decode_batch_wait_lp(dtk_ctx* ctx, int64_t* tokens_out /* [DTK_MAX_BATCH] */, float* logprob_out /* [DTK_MAX_BATCH] */,
                              float* sample_logprob_out /* [DTK_MAX_BATCH] */);
int  dtk_engine_read_lp(dtk_engine* e, int slot, int64_t* tokens_out, float* logprob_out, float* sample_logprob_out, int cap,
                        int32_t* n_out, int32_t* state_out, int timeout_ms);
int  dtk_engine_set_wait_lp_op(dtk_engine* e, int (*wait_lp)(void* dev, int64_t* tokens_out, float* logprob_out, float* sample_logprob_out));
int  dtk_op_sample_lp(dtk_ctx* ctx, const float* logits, int V, int step, int64_t* token_out, float* filtered_probs_out,
                      float* lp_out /* [2] */);

/* Top-k alternatives (additive, ABI 7): the k <= DTK_MAX_TOP most likely tokens of a position next to the one token the calls above
 * report.  For raw logits z[0 .. V) — the bf16-rounded values of the scoring lm_head, or the fp32 row a decode step samples from;
 * before suppression lists, temperature, top-k and top-p — the vocabulary is ordered by z descending, token id ascending on exact ties;
 * top-k = the first k entries as (id, logprob = z[id] - logsumexp(z)), with the logsumexp of the call's own lse / logprob.  Entry 0 is
 * the call's argmax; an entry whose id is the target (or the sampled token) carries that token's logprob, bit for bit.  1 <= k <= V.
 *   dtk_score_top, dtk_score_packed_top (+ _text)   the call without `_top` + k, top_ids_out, top_logprob_out ([rows][k], rows as
 *                             logprob_out).  k = 0 with both NULL is exactly the call without `_top`.  No [T][V] buffer: a selection
 *                             kernel picks, from the log-softmax records, the k 128-column tiles whose best elements come first and
 *                             computes only their logits again (same MFMA chain, same bits).
 *   dtk_op_score_top          dtk_op_score + the same, + top_z_out (the entries' z; may be NULL); k <= N
 *   dtk_set_option(ctx, "top_logprobs", k)   default 0, per context; needs "logprobs" = 1 (which cannot be switched off while k > 0); a change
 *                             of value is refused in the states that refuse "logprobs" and drops the captured decode graphs.  Every decode
 *                             step then runs one more kernel in front of its sampler and two more D2H copies; with 0 the steps are what
 *                             they are without the option.
 *   dtk_decode_wait_top       dtk_decode_wait_lp + top_ids_out / top_logprob_out [DTK_MAX_TOP]: entries >= k are (-1, NaN); a forced
 *                             token has (-1, NaN) throughout
 *   dtk_decode_batch_wait_top dtk_decode_batch_wait_lp + [DTK_MAX_BATCH][DTK_MAX_TOP] of the same; (-1, NaN) for slots that took no part
 *   dtk_set_option(ctx, "top_kernel", v)     which kernel selects a step's records: 1 = k_top_logits, one block per sequence that walks
 *                             the row k times; 2 = k_top_slice + k_top_merge, the row cut into slices of "top_slice" logits that are
 *                             loaded once into registers, the slices' k first entries merged by a second launch; 0 (default) = 2 where the
 *                             row has more than one slice (V > 8192; measured faster at V = 32 256 and 128 256), else 1.  The order is total, so the records are
 *                             the same bits either way.  "top_slice" (default 8192 = the most; at most 32 slices of the vocabulary) is
 *                             there for tests.  Both are refused in the states that refuse "top_logprobs" and drop the captured graphs.
 *   dtk_op_top_logits         the selection alone on host rows [rows][V] (rows <= DTK_MAX_BATCH, V <= 262 144, k <= min(V, DTK_MAX_TOP)),
 *                             through the shipped launcher: kernel 1 or 2, L = the slice of kernel 2.  active / forced [rows] or NULL
 *                             (all active / none forced): an inactive row's outputs are not written, a forced row gets (-1, NaN) in
 *                             its first k entries.  ids_out / z_out [rows][DTK_MAX_TOP] are in/out: entries >= k keep the caller's bytes.
 * The engines deliver them too (dtk_engine_read's and dtk_engine_read_lp's records are unchanged):
 *   dtk_engine_read_top       dtk_engine_read_lp + top_ids_out / top_logprob_out [cap][DTK_MAX_TOP]; the i-th record belongs to the i-th
 *                             token returned.  A record is (-1, NaN) beyond k, for a forced token and for tokens produced before
 *                             collection began.  Of a guided sequence the records are its conditional slot's, i.e. of the guided
 *                             distribution (the selection runs behind the mix).  The engine of dtk_engine_create collects through
 *                             dtk_decode_batch_wait_top while its context's "top_logprobs" is > 0 (switch it before the first join); an
 *                             engine of dtk_engine_create_ops through the op given to dtk_engine_set_wait_top_op (the contract of
 *                             dtk_decode_batch_wait_top; it then replaces ops.wait and the wait_lp op).  DTK_ERR_ARG while the engine
 *                             collects none. */
#define DTK_MAX_TOP 8
int  dtk_op_top_logits(dtk_ctx* ctx, const float* logits /* [rows][V] */, int rows, int V, int k, int kernel, int L, const int32_t* active,
                       const int32_t* forced, int32_t* ids_out /* [rows][DTK_MAX_TOP] */, float* z_out /* [rows][DTK_MAX_TOP] */);
int  dtk_engine_read_top(dtk_engine* e, int slot, int64_t* tokens_out, float* logprob_out, float* sample_logprob_out,
                         int32_t* top_ids_out /* [cap][DTK_MAX_TOP] */, float* top_logprob_out /* [cap][DTK_MAX_TOP] */, int cap,
                         int32_t* n_out, int32_t* state_out, int timeout_ms);
int  dtk_engine_set_wait_top_op(dtk_engine* e, int (*wait_top)(void* dev, int64_t* tokens_out, float* logprob_out, float* sample_logprob_out,
                                                               int32_t* top_ids_out, float* top_logprob_out));
int  dtk_score_top(dtk_ctx* ctx, const int64_t* ids, int T, const float* pixels, uint64_t image_key, uint32_t flags, int first,
                   float* logprob_out, int32_t* argmax_out, float* lse_out, int k, int32_t* top_ids_out, float* top_logprob_out);
int  dtk_score_top_text(dtk_ctx* ctx, const int64_t* ids, int T, const float* pixels, uint64_t image_key, const int64_t* text_ids, int T_text,
                        uint64_t text_key, uint32_t flags, int first, float* logprob_out, int32_t* argmax_out, float* lse_out,
                        int k, int32_t* top_ids_out, float* top_logprob_out);
int  dtk_score_packed_top(dtk_ctx* ctx, const int64_t* prefix_ids, int P, const float* pixels, uint64_t image_key, uint32_t flags,
                          const int64_t* cand_ids, const int32_t* cand_len, int N, float* logprob_out, int32_t* argmax_out, float* lse_out,
                          int k, int32_t* top_ids_out, float* top_logprob_out);
int  dtk_score_packed_top_text(dtk_ctx* ctx, const int64_t* prefix_ids, int P, const float* pixels, uint64_t image_key, const int64_t* text_ids,
                               int T_text, uint64_t text_key, uint32_t flags, const int64_t* cand_ids, const int32_t* cand_len, int N,
                               float* logprob_out, int32_t* argmax_out, float* lse_out, int k, int32_t* top_ids_out, float* top_logprob_out);
int  dtk_op_score_top(dtk_ctx* ctx, const uint16_t* Xn, const uint16_t* W, const int32_t* targets, int M, int N, int K, int flags,
                      float* logprob_out, float* lse_out, int32_t* argmax_out, float* zmax_out, int k, int32_t* top_ids_out,
                      float* top_logprob_out, float* top_z_out);
int  dtk_decode_wait_top(dtk_ctx* ctx, int64_t* token_out, float* lp_out /* [2] */, int32_t* top_ids_out /* [DTK_MAX_TOP] */,
                         float* top_logprob_out /* [DTK_MAX_TOP] */);
int  dtk_decode_batch_wait_top(dtk_ctx* ctx, int64_t* tokens_out /* [DTK_MAX_BATCH] */, float* logprob_out /* [DTK_MAX_BATCH] */,
                               float* sample_logprob_out /* [DTK_MAX_BATCH] */, int32_t* top_ids_out /* [DTK_MAX_BATCH][DTK_MAX_TOP] */,
                               float* top_logprob_out /* [DTK_MAX_BATCH][DTK_MAX_TOP] */);

/* min_p and epsilon_cutoff (additive, ABI 7).  HF's warper order is temperature -> top-k -> top-p -> min-p -> (typical) -> epsilon; the
 * sampler's chain is now suppression lists -> temperature -> top-k -> top-p -> min-p -> epsilon -> draw, everything up to top-p (the total
 * its threshold is taken from included) as before.  kept_total, the draw and sample_logprob are over the final set; logprob and the top-k
 * records are over the raw logits and do not change; a greedy configuration ignores both values.
 *   dtk_set_sampling_ext / dtk_set_sampling_slot_ext   called AFTER dtk_set_sampling / dtk_set_sampling_slot, which reset both values
 *                             to 0 (a caller that knows nothing of them gets what it always got).  DTK_ERR_ARG outside the ranges or on NaN.
 *                             A context none of whose sequences has a value set runs the sampler kernels it ran before the values
 *                             existed; the first sequence that sets one makes the next step re-capture its graph with the kernels that
 *                             read them (values then change without a re-capture).
 *   dtk_op_sample_ext         dtk_op_sample_lp under the context's configuration with the call's own ext; lp_out may be NULL.
 *   dtk_engine_submit_ext     dtk_engine_submit (text_ids == NULL) or dtk_engine_submit_text whose sequence carries ext (copied at
 *                             submit): the loop applies it right after the join's set_sampling_slot.  dtk_engine_create wires dtk_set_sampling_slot_ext itself; an engine of
 *                             dtk_engine_create_ops gets the op through dtk_engine_set_sampling_ext_op, and without one a join whose ext
 *                             is not 0 / 0 fails in submit with DTK_ERR_STATE.  With the op every join calls it — a join without ext
 *                             with 0 / 0 — so a slot never inherits its previous sequence's values. */
int  dtk_set_sampling_ext(dtk_ctx* ctx, const dtk_sampling_ext* x);
int  dtk_set_sampling_slot_ext(dtk_ctx* ctx, int slot, const dtk_sampling_ext* x);
int  dtk_op_sample_ext(dtk_ctx* ctx, const float* logits, int V, int step, int64_t* token_out, float* filtered_probs_out,
                       float* lp_out /* [2] or NULL */, const dtk_sampling_ext* x);
int  dtk_engine_submit_ext(dtk_engine* e, dtk_join* j, const dtk_sampling_ext* x, const int64_t* text_ids, int n_text, uint64_t text_key,
                           uint64_t* ticket_out);
int  dtk_engine_set_sampling_ext_op(dtk_engine* e, int (*set_sampling_slot_ext)(void* dev, int slot, const dtk_sampling_ext* x));

/* presence_penalty and frequency_penalty (additive, ABI 7): the OpenAI / vLLM pair, a transform of the raw logits in front of the whole
 * sampler chain.  Per sequence: presence pp and frequency fp, finite, in [-2, 2] (0 / 0 = off), and penalty_start s >= 0.  c[i] = the
 * occurrences of id i among the sequence's tokens at positions [s, next_pos): the prompt from s on and every token sampled or forced
 * since — a property of the token list, however the slot got there (prefill with or without DTK_PREFILL_REUSE_PREFIX, dtk_kv_fork,
 * dtk_resume_slot, an engine's join).  For c[i] > 0:  z'[i] = z[i] - (float)((double)pp + (double)fp * (double)c[i]), one fp32
 * subtraction on the raw fp32 logit; c[i] == 0 leaves the bits of z[i].  z' replaces z in front of the suppression lists (-inf stays
 * -inf), the temperature, top-k, top-p, min-p, epsilon and the draw; greedy takes the arg-max of z' (lowest id on ties).  logprob, the
 * top-k records and their logsumexp stay over the RAW logits (what dtk_score reports); sample_logprob and filtered_probs_out are over the
 * final kept set of the penalised chain.  A sequence with 0 / 0 draws what it draws alone, whatever its company in a batched step.
 * The counts are uint16 tables on the device (allocated with the first non-zero value: refused with DTK_ERR_RANGE if max_positions >=
 * 65536), rebuilt wherever the host redefines the sequence and advanced by one kernel behind the step's sampler.
 *   dtk_set_penalties / dtk_set_penalties_slot   called AFTER dtk_set_sampling / dtk_set_sampling_slot, which reset the three values to
 *                             0 / 0 / 0.  DTK_ERR_ARG outside the ranges or on NaN; DTK_ERR_STATE while steps of the sequence are unread.
 *                             A sequence that exists already gets its table rebuilt from its ids — a slot resumed by dtk_resume_slot
 *                             whose forced step has not been launched yet included, forced id and all — so the values may be set
 *                             before or after the call that defines the sequence.  (Set before it, as both engines do, the table
 *                             is built twice: once here from whatever the slot held, once by the prefill / fork / resume; each build
 *                             is a zero-fill, a copy of at most max_positions ids and a one-block kernel, queued on the stream.)
 *                             A context none of whose sequences has a value runs
 *                             the sampler kernels it ran before the penalties existed; the first that sets one makes the next step
 *                             re-capture its graph with the kernels that read them.
 *   dtk_op_sample_pen         dtk_op_sample_ext (x may be NULL: the context's own min_p / epsilon_cutoff) with the call's own values and a
 *                             token list whose multiset is the counts (ids in [0, V), at most 65535).
 *   dtk_token_counts          diagnostic: the V first counts the sequence's next step will read (slot -1: the single sequence); zeros
 *                             while no sequence of the context ever had a value, for a sequence without values, and after whatever
 *                             leaves a sequence undefined (weights or an adapter loaded, dtk_score_packed).
 *   dtk_engine_submit_pen     dtk_engine_submit_ext (x may be NULL) whose sequence also carries the three values: the loop applies them
 *                             right after the join's sampling calls.  dtk_engine_create wires dtk_set_penalties_slot itself; an engine of
 *                             dtk_engine_create_ops gets the op through dtk_engine_set_penalties_op, and without one a join whose values
 *                             are not 0 / 0 fails in submit with DTK_ERR_STATE.  With the op every join calls it — a join without
 *                             values with 0 / 0 / 0 — so a slot never inherits its previous sequence's values. */
int  dtk_set_penalties(dtk_ctx* ctx, float presence, float frequency, int start);
int  dtk_set_penalties_slot(dtk_ctx* ctx, int slot, float presence, float frequency, int start);
int  dtk_op_sample_pen(dtk_ctx* ctx, const float* logits, int V, int step, int64_t* token_out, float* filtered_probs_out,
                       float* lp_out /* [2] or NULL */, const dtk_sampling_ext* x /* or NULL */, float presence, float frequency,
                       const int64_t* counted_ids, int n_counted);
int  dtk_token_counts(dtk_ctx* ctx, int slot, uint16_t* out, int V);
int  dtk_engine_submit_pen(dtk_engine* e, dtk_join* j, const dtk_sampling_ext* x /* or NULL */, float presence, float frequency, int start,
                           const int64_t* text_ids, int n_text, uint64_t text_key, uint64_t* ticket_out);
int  dtk_engine_set_penalties_op(dtk_engine* e, int (*set_penalties_slot)(void* dev, int slot, float presence, float frequency, int start));

/* DRY ("don't repeat yourself"; additive, ABI 7): a penalty on the token that would extend a verbatim repetition of the sequence's own
 * recent text, growing exponentially with the length of the repetition.  Per sequence:
 *   multiplier m   finite, in [0, 100]; 0 = off            base b            finite, in [1, 8]
 *   allowed_length a   in [1, 64]                           start s >= 0      with the meaning of penalty_start
 *   breakers       at most DTK_DRY_MAX_BREAKERS ids in [0, V), the set B
 * Penalty table (host, IEEE double, repeated multiplication; the device only looks it up): pen[L] = 0 for L < a; p = (double)m; for
 * L = a .. DTK_DRY_MAX_MATCH: pen[L] = (float)min(p, 1e30), p *= (double)b.
 * History h[0, n): the sequence's ids at positions [s, next_pos) — the prompt from s on and every token sampled or forced since; a
 * property of the token list, however the slot got there.  If n < 2 or h[n-1] in B nothing is penalised.  Otherwise, for every i in
 * [0, n-2] with h[i] == h[n-1] and h[i+1] not in B:  L(i) = the largest L in [1, 64] such that for every k in [1, L): i-k >= 0,
 * h[i-k] == h[n-1-k] and h[n-1-k] not in B (overlap with the tail is allowed).  M[t] = max L(i) over the i with h[i+1] == t, else 0.
 * z'[t] = z[t] - pen[M[t]] where M[t] >= a, else the untouched bits of z[t]; behind the presence / frequency subtraction where both
 * are on (two fp32 subtractions in that order), in front of the suppression lists, the temperature, top-k, top-p, min-p, epsilon and
 * the draw; greedy takes the arg-max of z' (lowest id on ties).  logprob, the top-k records and their logsumexp stay over the RAW
 * logits; sample_logprob and filtered_probs_out are over the final kept set.  A sequence with m = 0 reads no DRY state and draws what it
 * draws alone.  State (allocated with the first m != 0, together with the penalties' per-sequence records, not their tables): an int32 history
 * and its length per sequence, rebuilt wherever the host redefines the sequence (the places of the count tables) and appended to by the
 * trailing kernel behind the sampler; a byte table of M per sequence, written by k_dry_scan in front of every step's sampler.
 *   dtk_set_dry / dtk_set_dry_slot   called AFTER dtk_set_sampling / dtk_set_sampling_slot, which reset DRY to off.  DTK_ERR_ARG outside
 *                             the ranges or on NaN; DTK_ERR_STATE while steps of the sequence are unread.  A sequence that exists
 *                             already gets its history rebuilt from its ids, a resumed slot's pending forced id included.
 *   dtk_dry_history           diagnostic: the length of the history the sequence's next scan will read (slot -1: the single sequence),
 *                             its first n_max ids to ids_out; 0 while the feature is off; a negative error code otherwise.
 *   dtk_dry_state_bytes       diagnostic: the device and pinned bytes the DRY state holds; 0 until a sequence of the context has had m != 0.
 *   dtk_op_dry_scan           k_dry_scan over a given history (d->start is not used); with history2 a second scan on the state the
 *                             first left.  Returns the number of ids with M != 0 in the whole table behind the last scan; the first
 *                             n_max, ascending, go to ids_out / m_out.  A negative error code otherwise.
 *   dtk_op_sample_dry         dtk_op_sample_pen with a history and a dtk_dry: scan, then the sampler.
 *   dtk_engine_submit_dry     dtk_engine_submit_pen whose sequence also carries a dtk_dry record (d; NULL: off); dtk_engine_create wires
 *                             dtk_set_dry_slot itself, an engine of dtk_engine_create_ops gets the op through dtk_engine_set_dry_op, and
 *                             without one a join with m != 0 fails in submit with DTK_ERR_STATE.  With the op every join calls it. */
#define DTK_DRY_MAX_MATCH 64
#define DTK_DRY_MAX_BREAKERS 16
typedef struct dtk_dry {
  float multiplier;
  float base;
  int32_t allowed_length;
  int32_t start;
  int32_t n_breakers;
  int32_t breakers[DTK_DRY_MAX_BREAKERS];
} dtk_dry;
int  dtk_set_dry(dtk_ctx* ctx, const dtk_dry* d);
int  dtk_set_dry_slot(dtk_ctx* ctx, int slot, const dtk_dry* d);
int  dtk_dry_history(dtk_ctx* ctx, int slot, int32_t* ids_out, int n_max);
int64_t dtk_dry_state_bytes(const dtk_ctx* ctx);
int  dtk_op_dry_scan(dtk_ctx* ctx, int V, const int64_t* history, int n_history, const int64_t* history2 /* or NULL */, int n_history2,
                     const dtk_dry* d, int32_t* ids_out, uint8_t* m_out, int n_max);
int  dtk_op_sample_dry(dtk_ctx* ctx, const float* logits, int V, int step, int64_t* token_out, float* filtered_probs_out,
                       float* lp_out /* [2] or NULL */, const dtk_sampling_ext* x /* or NULL */, float presence, float frequency,
                       const int64_t* counted_ids, int n_counted, const int64_t* history, int n_history, const dtk_dry* d);
int  dtk_engine_submit_dry(dtk_engine* e, dtk_join* j, const dtk_sampling_ext* x /* or NULL */, float presence, float frequency, int start,
                           const dtk_dry* d /* or NULL */, const int64_t* text_ids, int n_text, uint64_t text_key, uint64_t* ticket_out);
int  dtk_engine_set_dry_op(dtk_engine* e, int (*set_dry_slot)(void* dev, int slot, const dtk_dry* d));

/* Length control and logit bias (additive, ABI 7): min_new_tokens, an exponential decay of the EOS logit with the length, and a bias
 * per token id.  Transforms of the raw logits around the penalties, per sequence, all off by default.  cur = the number of tokens the
 * sequence holds when a token is sampled (DecState::next_pos), n = cur - start, E = the sequence's eos_ids.  For a raw logit z[i]:
 *   1. bias     b[i] != 0: z1 = z[i] + b[i], one fp32 addition; b[i] == 0: the untouched bits of z[i].  At most DTK_BIAS_MAX ids in
 *               [0, V), no id twice, values finite in [-100, 100].
 *   2. dtk_set_penalties, then dtk_set_dry, on z1, unchanged.
 *   3. decay    i in E and n > decay_start: with k = n - decay_start, z3 = fl(z2 + fl(|z2| * m[k])), two fp32 roundings, never an fma;
 *               m[k] = min((float)(pow(decay_factor, k) - 1.0), 0x1p100f), a host-built table of max_positions + 1 floats (the
 *               device only looks it up).  decay_factor 0 = no decay; otherwise finite and > 0.
 *   4. minimum  i in E and n < min_new_tokens: -inf.
 *   5. the suppression lists, the temperature, top-k, top-p, min-p, epsilon and the draw; greedy takes the arg-max (lowest id on ties).
 * logprob, the top-k records and their logsumexp stay over the RAW logits.  decay_start >= min_new_tokens is required with a decay (the
 * two rules never meet: -inf + inf would be NaN); m saturates at 2^100 where pow would reach inf.  All of it is static for a sequence:
 * nothing is rebuilt when the host redefines one (prefill, fork, resume, prefix reuse), n follows the token list.  A sequence without
 * values reads no table and draws what it draws alone.  State (allocated with the first value that is set): one record per sequence,
 * a float [max_positions + 1] decay table per sequence with the first decay, a dense float [V] bias table per sequence with the first bias.
 *   dtk_set_length_control[_slot]  called AFTER dtk_set_sampling[_slot], which reset the rules to off.  DTK_ERR_ARG outside the ranges,
 *                             on NaN, on an EOS id outside [0, V); DTK_ERR_STATE while steps of the sequence are unread.
 *   dtk_set_logit_bias[_slot] likewise; n = 0 clears.  The table is filled by k_bias_scatter and cleared by re-zeroing the listed ids.
 *   dtk_logit_bias_table      diagnostic: the sequence's dense table (slot -1: the single sequence) to out[0, V); zeros while the
 *                             feature is off.  Returns the number of entries != 0, or a negative error code.
 *   dtk_op_sample_shape       dtk_op_sample_dry at sequence length cur (l->start is honoured: n = cur - l->start) with a dtk_length_ctl
 *                             and bias pairs: the PN sampler instantiations with every table, whatever the values are.
 *   dtk_engine_submit_shape   dtk_engine_submit_dry whose sequence also carries the two new records (NULL / 0: off); dtk_engine_create
 *                             wires the slot setters itself, an engine of dtk_engine_create_ops gets them through
 *                             dtk_engine_set_length_control_op / dtk_engine_set_logit_bias_op, and without one a join with values
 *                             fails in submit with DTK_ERR_STATE.  With the op every join calls it. */
#define DTK_BIAS_MAX 256
typedef struct dtk_length_ctl {
  int32_t min_new_tokens;
  int32_t decay_start;
  double  decay_factor;   /* a double: HF raises the Python float itself to the power k */
  int32_t start;
  int32_t n_eos;
  int32_t eos_ids[8];
} dtk_length_ctl;
int  dtk_set_length_control(dtk_ctx* ctx, const dtk_length_ctl* l);
int  dtk_set_length_control_slot(dtk_ctx* ctx, int slot, const dtk_length_ctl* l);
int  dtk_set_logit_bias(dtk_ctx* ctx, const int32_t* ids, const float* values, int n);
int  dtk_set_logit_bias_slot(dtk_ctx* ctx, int slot, const int32_t* ids, const float* values, int n);
int  dtk_logit_bias_table(dtk_ctx* ctx, int slot, float* out, int V);
int  dtk_op_sample_shape(dtk_ctx* ctx, const float* logits, int V, int step, int64_t* token_out, float* filtered_probs_out,
                         float* lp_out /* [2] or NULL */, const dtk_sampling_ext* x /* or NULL */, float presence, float frequency,
                         const int64_t* counted_ids, int n_counted, const int64_t* history, int n_history, const dtk_dry* d,
                         int cur, const dtk_length_ctl* l, const int32_t* bias_ids, const float* bias_values, int n_bias);
int  dtk_engine_submit_shape(dtk_engine* e, dtk_join* j, const dtk_sampling_ext* x /* or NULL */, float presence, float frequency, int start,
                             const dtk_dry* d /* or NULL */, const dtk_length_ctl* l /* or NULL */, const int32_t* bias_ids,
                             const float* bias_values, int n_bias, const int64_t* text_ids, int n_text, uint64_t text_key,
                             uint64_t* ticket_out);
int  dtk_engine_set_length_control_op(dtk_engine* e, int (*set_length_control_slot)(void* dev, int slot, const dtk_length_ctl* l));
int  dtk_engine_set_logit_bias_op(dtk_engine* e, int (*set_logit_bias_slot)(void* dev, int slot, const int32_t* ids, const float* values, int n));

/* Classifier-free guidance (additive, ABI 7): HF's UnbatchedClassifierFreeGuidanceLogitsProcessor for two batch slots that decode in
 * one step.  A pair is a conditional slot c and an unconditional slot u (two prompts, e.g. the sketch and an empty canvas).  In every
 * batched step, in front of everything else that reads the pending raw logits (the top-k records, bias, penalties, DRY, the length
 * rules, the suppression lists, temperature, top-k, top-p, min-p, epsilon; greedy included), row c is replaced in place by
 *     Lc = logsumexp(zc)   Lu = logsumexp(zu)   lc = zc[v] - Lc   lu = zu[v] - Lu   out[v] = g * (lc - lu) + lu
 * in fp32, every subtraction, multiplication and addition rounded on its own (never an fma), so a host that is given the device's
 * (Lc, Lu) reproduces out bit for bit.  Consequently a guided sequence's logprob, its top-k records and their logsumexp describe the
 * GUIDED distribution out[t] - logsumexp(out).  Behind the sampler slot u takes over the token slot c's chain chose (its DecState, the
 * gathered embedding, the step's ring entries): one token per pair per step, both slots report it.  Slot u's own sampling state is
 * not consulted; keep it at neutral greedy sampling with no tables.  The two launches in front (k_cfg_lse, k_cfg_mix: grid (slice,
 * pair), the slice count a function of V alone, no atomics) and the one behind (k_cfg_follow) exist only in the steps of a context
 * with a pair: without one the step launches exactly what it launched before, and nothing is allocated before the first pair.
 * Contexts without slots (tl-1.1b's head_dim 64, MXFP4) have no guidance.
 *   dtk_set_guidance   pairs two distinct decoding slots (scale finite in [0, 100]); the same pair again changes its scale;
 *                      uncond_slot < 0 or scale == 1 dissolves the pair cond_slot heads (no pair: DTK_OK).  DTK_ERR_ARG for a slot out of
 *                      range, a slot already in another pair, equal slots, a scale outside the range or not finite; DTK_ERR_STATE while a
 *                      batch step is in flight.  At most DTK_MAX_BATCH / 2 pairs.  A pair is static for a sequence: dtk_prefill_slot,
 *                      dtk_resume_slot and dtk_kv_fork leave it alone.  Every change re-captures the batched step, unless the
 *                      pairs stand (dtk_reserve_guidance).
 *   dtk_reserve_guidance   standing pairs: from here on the captured batched steps (three tile counts, three multi-vector widths) launch
 *                      the three kernels with n_pairs as the pair dimension of their grids whatever the number of live pairs; a block
 *                      learns from the device table whether its entry is live (an unused entry has cond < 0 and returns before it reads
 *                      anything else).  While the live pairs fit, dtk_set_guidance (form, dissolve, new scale) only writes the table
 *                      and no capture is dropped; a pair beyond the reservation behaves as without one.  A live pair's blocks compute
 *                      what they compute without a reservation, bit for bit.  n_pairs in 0 .. DTK_MAX_BATCH / 2 (DTK_ERR_ARG); 0 ends
 *                      the reservation and, with no live pair, frees the table.  DTK_ERR_STATE while a batch step is in flight.  It
 *                      allocates what the first dtk_set_guidance allocates.  A context that never calls it behaves as before.
 *   dtk_batch_graph_captures   captures of a batched step since the context was created (a re-capture shows as an increment).
 *   resumed pairs      dtk_resume_slot on both slots of a pair: in the step that forwards the two last prompt tokens k_cfg_lse and
 *                      k_cfg_mix skip the pair (its rows are stale or were never written) and k_cfg_follow hands nothing over: each
 *                      slot reports its own forced token with NaN log-probabilities; (Lc, Lu) keep their earlier values.
 *   dtk_get_guidance   diagnostic: slot's partner (-1: none), whether slot is the conditional one, the scale (1 without a pair) and
 *                      lse_out[2] = (Lc, Lu) of the pair's last step (NaN without a pair; meaningful once the pair has decoded a step since
 *                      the last dtk_set_guidance that changed the set of pairs); any out pointer may be NULL.
 *   dtk_decode_batch_launch   refuses (DTK_ERR_ARG, nothing launched) a step in which exactly one slot of a pair is active, or in which
 *                      exactly one slot of an active pair forwards a forced token (resume both slots or prefill both).
 *   dtk_op_cfg_mix     the two mixing kernels in the launch shape the step uses for that V, on two rows at stride V of the op scratch:
 *                      out[V] and lse_out[2] = (Lc, Lu).  2 <= V <= 262 144.  The 256 bytes behind out are checked (DTK_ERR_STATE).
 *   dtk_bench_cfg      tools/bench_cfg.py: HIP events around reps (1 .. 64) back-to-back launches on the context's own pairs and rows:
 *                      avg_us[0] = k_cfg_lse + k_cfg_mix, avg_us[1] = k_cfg_follow.  The conditional slots' pending rows are mixed over
 *                      and over: prefill the pairs again before decoding on. */
int  dtk_set_guidance(dtk_ctx* ctx, int cond_slot, int uncond_slot, float scale);
int  dtk_get_guidance(dtk_ctx* ctx, int slot, int* partner_out, int* is_cond_out, float* scale_out, float* lse_out /* [2] */);
int  dtk_op_cfg_mix(dtk_ctx* ctx, const float* zc, const float* zu, int V, float scale, float* out /* [V] */, float* lse_out /* [2] */);
int  dtk_bench_cfg(dtk_ctx* ctx, int reps, float* avg_us /* [2] */);
int  dtk_reserve_guidance(dtk_ctx* ctx, int n_pairs);
int64_t dtk_batch_graph_captures(const dtk_ctx* ctx);

/* Guided sequences in the engine's slots (additive, ABI 7; dtk_abi_struct_size(18) = sizeof(dtk_guided)).  A guided sequence is ONE
 * command that carries two joins: `cond`, the sequence itself (everything a dtk_join says), and `uncond`, the negative branch's own plan
 * — slot, ids, pixels, image key, try_resume and the prefix plan; its sampling, budget, stop ids, flush fields and candidates are not
 * used (n_candidates must be 0 in both: a pair is resumed where its owner left it).  dtk_engine_submit_guided takes the arguments of
 * dtk_engine_submit_shape, which all describe the conditional slot; the unconditional slot gets neutral greedy sampling and no tables.
 *   joining    both slots must be free, distinct decoding slots.  Pairs of earlier sequences that still hold either slot are dissolved
 *              first (so are those an unguided join re-uses).  The two joins execute back to back with no step in flight.  The pair
 *              resumes in place only if BOTH slots hold their prompt (dtk_slot_lcp >= n - 1 under each one's own key) and both joins ask
 *              for it; otherwise both take their non-resume plan.  Then set_guidance(cond, uncond, scale).  A failure anywhere leaves no
 *              pair and both slots free; cond->error_out has the text, cond->how_out / uncond->how_out each join's way.
 *   stepping   the unconditional slot is a follower: it is launched and stopped with its leader (the budget is bounded by the smaller
 *              room of the two slots), its tokens are not delivered, and dtk_engine_read / _read_lp / _leave on it return DTK_ERR_ARG.
 *              Every collected step checks that both slots report the same token; a difference stops the engine (dtk_engine_last_error
 *              names the pair).  The forced tokens of a resumed pair are dropped unseen.
 *   ending     a stop id, the budget or dtk_engine_leave(cond) ends both at once; a step still in flight counts both slots as wasted.
 *              dtk_engine_stats: tokens_out, joins and resumed count a pair once.  The device's pair is dissolved by the next join
 *              that uses one of its slots (a pair with neither slot active launches nothing).
 * Engines from dtk_engine_create_ops get the device's pairing through dtk_engine_set_guidance_op (the signature of dtk_set_guidance;
 * cond, -1, 1 dissolves); without it dtk_engine_submit_guided fails with DTK_ERR_STATE and says so.  dtk_engine_create wires
 * dtk_set_guidance itself. */
typedef struct dtk_guided {
  dtk_join* cond;                   /* the sequence's join                                                                    */
  dtk_join* uncond;                 /* the negative branch's plan                                                             */
  const int64_t* uncond_text_ids;   /* the negative branch's own text (the adapter), or NULL                                   */
  int32_t n_uncond_text;
  float   scale;                    /* finite, in [0, 100], not 1                                                              */
  uint64_t uncond_text_key;
} dtk_guided;
int  dtk_engine_submit_guided(dtk_engine* e, const dtk_guided* g, const dtk_sampling_ext* x /* or NULL */, float presence, float frequency,
                              int start, const dtk_dry* d /* or NULL */, const dtk_length_ctl* l /* or NULL */, const int32_t* bias_ids,
                              const float* bias_values, int n_bias, const int64_t* text_ids, int n_text, uint64_t text_key,
                              uint64_t* ticket_out);
int  dtk_engine_set_guidance_op(dtk_engine* e, int (*set_guidance)(void* dev, int cond_slot, int uncond_slot, float scale));

/* ---- Prompt-lookup speculative decoding of slot 0 in the multi-vector step (additive, ABI 7) --------------------------
 * Between dtk_spec_begin and dtk_spec_end one step of a multi-vector context (2..5 slots) decodes up to K + 1 tokens of the sequence in
 * SLOT 0: the step's NV = K + 1 vectors (2 vectors for K = 1, the 4-vector step for K = 2 | 3) are consecutive positions of that one
 * sequence, all in slot 0's key/value cache.  Vector 0 forwards the last accepted token, vector i the draft d_i; the next step's sampler
 * launch runs over the NV pending logits rows with slot 0's sampling record and draw index c + i for row i, k_spec_accept keeps the
 * leading rows whose sampled token equals the draft the next vector forwarded (+ the first that does not), and k_spec_draft makes the
 * next drafts.  Every GEMV, attention and sampler launch of a row is the instantiation a plain dtk_decode_batch_launch step of slot 0
 * runs (only launch arguments differ), and a slot's result in that family depends neither on its index nor on its neighbours, so the
 * tokens and log-probabilities are, bit for bit, those of plain steps of slot 0 on the same context.  Rows a rejected draft wrote beyond
 * the accepted position are dead: the next step overwrites them before anything reads them.
 *   dtk_spec_begin      K = 1..3 drafts per step; max_ngram = 1..DTK_SPEC_MAX_NGRAM; source = DTK_SPEC_LOOKUP (HF's
 *                       PromptLookupCandidateGenerator over the sequence's ids on the device, prompt and image placeholders included: for
 *                       n = min(max_ngram, len - 1) down to 1 the first window, in ascending index, that equals the last n ids and is not
 *                       the tail itself gives its continuation, at most K ids; no match: no drafts) or DTK_SPEC_TABLE (an id per absolute
 *                       position from dtk_spec_set_drafts, -1 = none: tests decide acceptance with it).  Drafts are cut so that no vector's
 *                       position reaches max_positions.  Slot 0 must hold pending logits (a prefill, or plain steps that were read).
 *                       Refused before anything is allocated or changed — DTK_ERR_ARG: K or max_ngram or source out of range, fewer than
 *                       K + 1 decoding slots; DTK_ERR_STATE: a context outside the multi-vector family, kv_format mxfp8, a guided pair,
 *                       top_logprobs, a presence / frequency penalty, DRY, length control or a logit bias on any slot, a batch step in
 *                       flight, an engine holding the slots, a resumed slot 0 that has not forwarded its last prompt token yet.
 *                       Slots 1..K lose their pending logits (they need a prefill before they decode again) and keep their KV.  The
 *                       first call allocates 8 x max_positions bytes + a few records; a context that never calls it allocates nothing
 *                       and its steps launch what they launched before.
 *   dtk_spec_set_drafts the table of DTK_SPEC_TABLE: ids for positions [0, n), -1 beyond; DTK_ERR_STATE with a step in flight.
 *   dtk_spec_launch     one speculative step, captured like the batched steps (two more graphs: 2 and 4 vectors); up to DTK_MAX_INFLIGHT
 *                       in flight.  DTK_ERR_RANGE once length + 4 x (steps in flight) reaches max_positions: the host knows the
 *                       position only of the steps it has read.
 *   dtk_spec_wait       the oldest unread step: *n_out = 1..K + 1 accepted tokens in tokens_out[0 .. n) (-1 beyond), with their
 *                       (logprob, sample_logprob) when both pointers are given (needs option "logprobs"; NaN beyond n).
 *   dtk_spec_end        reads the steps still in flight, then leaves slot 0 holding exactly its first keep_len ids (1 .. its length) with
 *                       NO pending logits: a following prefill with DTK_PREFILL_REUSE_PREFIX recomputes one row, as after any truncation.
 *                       The caller decides where the sequence stops (EOS, a line end): tokens accepted past the stop are dropped here.
 * While slot 0 speculates dtk_decode_batch_launch / _wait, prefills into slots, dtk_kv_fork, dtk_resume_slot and dtk_set_guidance return
 * DTK_ERR_STATE.
 *   dtk_op_spec_lookup  k_spec_draft's lookup alone on ids[0, len) (len >= 0): drafts_out[4] (-1 beyond the count) and *n_out, cut as a
 *                       step whose vector 0 sits at position len - 1 of a max_positions = T_max context cuts them.
 *   dtk_bench_spec      tools/bench_spec.py: HIP events around reps (1 .. 64) back-to-back launches of k_spec_accept + k_spec_draft on the
 *                       speculating sequence's own state: *avg_us per pair.  The pairs move the position over stale records (never
 *                       beyond max_positions): afterwards the sequence is good for dtk_spec_end and a new prefill only.  With a corpus
 *                       set, k_spec_corpus runs between the two, as in a step.
 * A second draft source for DTK_SPEC_LOOKUP: a CORPUS of earlier programs (the boilerplate of every TikZ program, sibling rollouts of one
 * tree), a flat int32 array of at most DTK_SPEC_CORPUS_MAX entries that holds id sequences joined by a negative separator entry (-1).
 * With len ids h in the history, C corpus entries c and kmax = min(K, max_positions - 1 - (len - 1), NV - 1, 3):
 *     for n = min(max_ngram, len - 1) down to 1, tail = h[len - n : len]:
 *       1. the history, unchanged: the first idx in [0, len - n) with h[idx : idx + n] == tail gives h[idx + n : idx + n + kmax];
 *       2. otherwise the corpus: the first idx in [0, C - n) with c[idx : idx + n] == tail and c[idx + n] >= 0 gives
 *          c[idx + n : idx + n + kmax], cut in front of the first negative entry or at C;
 *     no match anywhere: no drafts.
 * A longer n-gram beats a shorter one whatever its source, at equal n the history wins, a window that contains a separator never matches
 * (tail ids are >= 0), a corpus window without a continuation id is skipped, and an empty corpus leaves the rule above.  The verify pass
 * decides every token, so a corpus changes how many tokens a step accepts and nothing else.  DTK_SPEC_TABLE ignores the corpus.
 *   dtk_spec_set_corpus  n = 0 clears.  DTK_ERR_ARG: an id >= the vocabulary size; DTK_ERR_RANGE: n > DTK_SPEC_CORPUS_MAX; DTK_ERR_STATE: a
 *                       speculative step in flight, or a context outside the multi-vector family.  The first non-empty call allocates
 *                       the corpus buffer (256 KiB) and 64 block results; a context that never calls it allocates nothing.  The corpus
 *                       persists over dtk_spec_begin / dtk_spec_end until it is cleared.  While one is set the captured speculative steps
 *                       hold one more kernel (k_spec_corpus, 64 blocks: one pass over the corpus per step): the change between none and
 *                       some drops the two speculative graphs (one re-capture each), replacing one corpus by another re-captures nothing.
 *   dtk_spec_corpus_len  the entries set (0: none).
 *   dtk_spec_counters   out[3] = the steps launched since dtk_spec_begin whose drafts (those the step made for the next one) came from the
 *                       history (or the table), from the corpus, from nowhere.  DTK_ERR_STATE with a step in flight.
 *   dtk_op_spec_lookup_corpus  dtk_op_spec_lookup with a corpus: k_spec_corpus + k_spec_draft on the op scratch in the step's launch
 *                       shape; + *source_out = DTK_SPEC_FROM_* and *ngram_out = the n that matched (0: none). */
enum { DTK_SPEC_LOOKUP = 0, DTK_SPEC_TABLE = 1 };
#define DTK_SPEC_MAX_NGRAM 16
#define DTK_SPEC_CORPUS_MAX 65536
#define DTK_SPEC_FROM_NONE 0
#define DTK_SPEC_FROM_HISTORY 1
#define DTK_SPEC_FROM_CORPUS 2
int  dtk_spec_begin(dtk_ctx* ctx, int K, int max_ngram, int source);
int  dtk_spec_set_drafts(dtk_ctx* ctx, const int32_t* table, int n);
int  dtk_spec_launch(dtk_ctx* ctx);
int  dtk_spec_wait(dtk_ctx* ctx, int64_t* tokens_out /* [4] */, int* n_out, float* logprob_out /* [4] or NULL */, float* sample_logprob_out /* [4] or NULL */);
int  dtk_spec_end(dtk_ctx* ctx, int keep_len);
int  dtk_op_spec_lookup(dtk_ctx* ctx, const int32_t* ids, int len, int K, int max_ngram, int T_max, int32_t* drafts_out /* [4] */, int* n_out);
int  dtk_bench_spec(dtk_ctx* ctx, int reps, float* avg_us);
int  dtk_spec_set_corpus(dtk_ctx* ctx, const int32_t* ids, int n);
int  dtk_spec_corpus_len(const dtk_ctx* ctx);
int  dtk_spec_counters(dtk_ctx* ctx, int64_t* out /* [3] */);
int  dtk_op_spec_lookup_corpus(dtk_ctx* ctx, const int32_t* ids, int len, const int32_t* corpus, int n_corpus, int K, int max_ngram, int T_max,
                               int32_t* drafts_out /* [4] */, int* n_out, int* source_out, int* ngram_out);

#ifdef __cplusplus
}
#endif
#endif /* DTK_H */
