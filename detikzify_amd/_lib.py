"""ctypes binding of include/dtk.h.  No CPU fallback: a missing library is a hard error."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "lib" / "libdtk_hip.so"

DTK_ABI_VERSION = 7          # include/dtk.h DTK_ABI_VERSION
DTK_VIT_BATCH = 8            # include/dtk.h: images per pass of dtk_vit_encode
DTK_F32, DTK_BF16, DTK_F16 = 0, 1, 2
DTK_ARCH_PROJ_NO_BIAS = 1   # include/dtk.h: dtk_config.reserved[3] flag
DTK_PREFILL_REUSE_PREFIX, DTK_PREFILL_REUSE_IMAGE = 1, 2
DTK_MAX_INFLIGHT = 4
DTK_MAX_BATCH = 64          # entries of the active / tokens_out arrays of dtk_decode_batch_*
DTK_MAX_TOP = 8             # most alternatives per position (dtk_score_top, dtk_set_option "top_logprobs")
DTK_EPI_BIAS, DTK_EPI_GELU, DTK_EPI_RESIDUAL, DTK_GEMM_NAIVE = 1, 2, 4, 256
DTK_EPI_GATED_RESIDUAL, DTK_EPI_GELU_ERF, DTK_EPI_GELU_TANH, DTK_GEMM_INPLACE = 8, 16, 32, 64      # dtk_op_gemm_ex
DTK_GEMM_WT = 512
DTK_GEMM_SL = 1024
DTK_GEMM_KSLICES_SHIFT = 12     # dtk_op_gemm: flags |= S << 12 selects the sliced-K family (include/dtk.h)


class DtkConfig(C.Structure):
    _fields_ = [
        ("hidden", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32), ("head_dim", C.c_int32),
        ("ffn", C.c_int32), ("vocab", C.c_int32), ("max_positions", C.c_int32),
        ("rms_eps", C.c_float), ("rope_theta", C.c_float), ("rope_factor", C.c_float),
        ("vit_dim", C.c_int32), ("vit_depth", C.c_int32), ("vit_heads", C.c_int32),
        ("vit_mlp", C.c_int32), ("vit_patch", C.c_int32), ("vit_image", C.c_int32),
        ("vit_feature_layer", C.c_int32), ("vit_ln_eps", C.c_float), ("vit_gelu_tanh", C.c_int32),
        ("concat_patches", C.c_int32), ("image_token_id", C.c_int32), ("attn_splits", C.c_int32),
        ("reserved", C.c_int32 * 7),
    ]


class DtkAdapterConfig(C.Structure):
    """dtk_adapter_config: the TikZero adapter and its embedding model (include/dtk.h, ABI 7)"""
    _fields_ = [
        ("every_n", C.c_int32), ("text_max", C.c_int32),
        ("hidden", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32), ("kv_heads", C.c_int32), ("head_dim", C.c_int32),
        ("ffn", C.c_int32), ("vocab", C.c_int32), ("rms_eps", C.c_float), ("rope_theta", C.c_float), ("rope_factor", C.c_float),
        ("rope_low_freq_factor", C.c_float), ("rope_high_freq_factor", C.c_float), ("rope_original_max_position", C.c_int32),
        ("reserved", C.c_int32 * 3),
    ]


class DtkSampling(C.Structure):
    _fields_ = [
        ("do_sample", C.c_int32), ("temperature", C.c_float), ("top_p", C.c_float),
        ("top_k", C.c_int32), ("seed", C.c_uint64),
        ("n_bad", C.c_int32), ("bad_ids", C.c_int32 * 8),
        ("n_begin_suppress", C.c_int32), ("begin_suppress_ids", C.c_int32 * 8),
        ("n_always_suppress", C.c_int32), ("always_suppress_ids", C.c_int32 * 8),
    ]


class DtkSamplingExt(C.Structure):
    """dtk_sampling_ext: min_p / epsilon_cutoff, set after dtk_set_sampling[_slot] (which resets both to 0)"""
    _fields_ = [("min_p", C.c_float), ("epsilon_cutoff", C.c_float), ("reserved", C.c_int32 * 6)]


DTK_DRY_MAX_MATCH = 64
DTK_DRY_MAX_BREAKERS = 16


class DtkDry(C.Structure):
    """dtk_dry: DRY of one sequence, set after dtk_set_sampling[_slot] (which resets it to off); multiplier 0 = off"""
    _fields_ = [("multiplier", C.c_float), ("base", C.c_float), ("allowed_length", C.c_int32), ("start", C.c_int32),
                ("n_breakers", C.c_int32), ("breakers", C.c_int32 * DTK_DRY_MAX_BREAKERS)]


DTK_BIAS_MAX = 256
DTK_LEN_MAX_EOS = 8


class DtkLengthCtl(C.Structure):
    """dtk_length_ctl: the length rules of one sequence, set after dtk_set_sampling[_slot] (which resets them to off); all 0 = off"""
    _fields_ = [("min_new_tokens", C.c_int32), ("decay_start", C.c_int32), ("decay_factor", C.c_double), ("start", C.c_int32),
                ("n_eos", C.c_int32), ("eos_ids", C.c_int32 * DTK_LEN_MAX_EOS)]


class DtkStats(C.Structure):
    _fields_ = [
        ("weight_bytes_per_token", C.c_uint64), ("kv_bytes_per_ctx_token", C.c_uint64),
        ("decode_steps", C.c_uint64), ("prefill_tokens", C.c_uint64), ("vit_images", C.c_uint64),
        ("last_prefill_ms", C.c_double), ("last_vit_ms", C.c_double),
        ("probe_kernel_ms_sum", C.c_double), ("probe_kernel_launches", C.c_uint64),
        ("probe_kernel_bytes", C.c_uint64), ("probe_event_pair_ms", C.c_double),
        ("last_batch_step_slots", C.c_uint32), ("device_errors", C.c_uint32),
        ("last_batch_step_fp8_mfma", C.c_uint32), ("w13_counts", C.c_uint32),
    ]


class DtkJoin(C.Structure):
    """dtk_join: one sequence handed to the native run loop (dtk_engine_join)"""
    _fields_ = [
        ("slot", C.c_int32), ("n_ids", C.c_int32), ("ids", C.c_void_p), ("pixels", C.c_void_p), ("image_key", C.c_uint64),
        ("try_resume", C.c_int32), ("n_candidates", C.c_int32), ("candidates", C.c_int32 * DTK_MAX_BATCH),
        ("prefix_len", C.c_int32), ("prefix_src", C.c_int32), ("prefix_src_whole", C.c_int32), ("prefix_encode", C.c_int32),
        ("prefix_in_place", C.c_int32), ("full_flags", C.c_int32), ("sampling", DtkSampling),
        ("max_new_tokens", C.c_int32), ("n_stop", C.c_int32), ("stop_ids", C.c_int64 * 8),
        ("flush_mode", C.c_int32), ("flush_max", C.c_int32), ("slot_out", C.c_int32), ("how_out", C.c_int32),
        ("error_out", C.c_char * 240),
    ]


class DtkGuided(C.Structure):
    """dtk_guided: a guided sequence for dtk_engine_submit_guided — the sequence's join, the negative branch's plan and text, the scale"""
    _fields_ = [("cond", C.POINTER(DtkJoin)), ("uncond", C.POINTER(DtkJoin)), ("uncond_text_ids", C.c_void_p),
                ("n_uncond_text", C.c_int32), ("scale", C.c_float), ("uncond_text_key", C.c_uint64)]


class DtkEngineStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("steps", "tokens_out", "joins", "resumed", "steps_below_half_occupancy", "host_bound_steps",
                                          "reader_wakeups", "wasted_slot_steps")] + \
               [(n, C.c_double) for n in ("wait_s", "launch_s", "join_s", "idle_s", "drain_s", "first_launch_t", "last_collect_t")]


_I32P, _I64P = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


class DtkEngineOps(C.Structure):
    """dtk_engine_ops: the device under the native run loop (the CPU tests script one in Python)"""
    LAUNCH = C.CFUNCTYPE(C.c_int, C.c_void_p, _I32P)
    WAIT = C.CFUNCTYPE(C.c_int, C.c_void_p, _I64P)
    PREFILL = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, _I64P, C.c_int, C.c_void_p, C.c_uint64, C.c_int)
    SAMPLING = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(DtkSampling))
    FORK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int)
    LCP = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, _I64P, C.c_int, C.c_uint64, C.POINTER(C.c_int))
    RESUME = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, _I64P, C.c_int, C.c_uint64)
    CTXLEN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int)
    LASTERR = C.CFUNCTYPE(C.c_void_p, C.c_void_p)     # (const char*: the callee owns the text)
    # not a field: dtk_engine_set_prefill_text_op's argument (dev, slot, ids, T, pixels, image_key, text_ids, n_text, text_key, flags)
    PREFILL_TEXT = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, _I64P, C.c_int, C.c_void_p, C.c_uint64, _I64P, C.c_int, C.c_uint64, C.c_int)
    # not a field: dtk_engine_set_wait_lp_op's argument (dev, tokens_out[64], logprob_out[64], sample_logprob_out[64])
    WAIT_LP = C.CFUNCTYPE(C.c_int, C.c_void_p, _I64P, C.POINTER(C.c_float), C.POINTER(C.c_float))
    # not a field: dtk_engine_set_wait_top_op's argument (WAIT_LP's + top_ids_out[64][8], top_logprob_out[64][8])
    WAIT_TOP = C.CFUNCTYPE(C.c_int, C.c_void_p, _I64P, C.POINTER(C.c_float), C.POINTER(C.c_float), _I32P, C.POINTER(C.c_float))
    # not a field: dtk_engine_set_sampling_ext_op's argument (dev, slot, ext)
    SAMPLING_EXT = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(DtkSamplingExt))
    # not a field: dtk_engine_set_penalties_op's argument (dev, slot, presence, frequency, start)
    PENALTIES = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int)
    # not a field: dtk_engine_set_dry_op's argument (dev, slot, dry)
    DRY = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(DtkDry))
    # not fields: dtk_engine_set_length_control_op's (dev, slot, ctl) and dtk_engine_set_logit_bias_op's (dev, slot, ids, values, n)
    LENGTH_CTL = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(DtkLengthCtl))
    LOGIT_BIAS = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int)
    # not a field: dtk_engine_set_guidance_op's argument (dev, cond_slot, uncond_slot, scale)
    GUIDANCE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float)
    _fields_ = [
        ("dev", C.c_void_p), ("launch", LAUNCH), ("wait", WAIT), ("prefill_slot", PREFILL), ("set_sampling_slot", SAMPLING),
        ("kv_fork", FORK), ("slot_lcp", LCP), ("resume_slot", RESUME), ("context_len_slot", CTXLEN), ("last_error", LASTERR),
        ("max_positions", C.c_int32), ("decode_slots", C.c_int32),
    ]


DTK_JOIN_FULL, DTK_JOIN_FORK_TAIL, DTK_JOIN_FORK_WHOLE, DTK_JOIN_RESUMED, DTK_JOIN_IN_PLACE = range(5)
DTK_SEQ_RUNNING, DTK_SEQ_FINISHED, DTK_SEQ_LEFT = 1, 2, 3

# every symbol include/dtk.h declares: (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "dtk_abi_version": (C.c_int, []),
    "dtk_abi_struct_size": (C.c_int, [C.c_int]),
    "dtk_last_error": (C.c_char_p, [_P]),
    "dtk_create": (C.c_int, [C.POINTER(DtkConfig), C.c_int, C.POINTER(_P)]),
    "dtk_destroy": (None, [_P]),
    "dtk_load_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "dtk_read_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "dtk_fill_synthetic": (C.c_int, [_P, C.c_uint64]),
    "dtk_num_tensors": (C.c_int, [_P]),
    "dtk_tensor_name": (C.c_char_p, [_P, C.c_int]),
    "dtk_tensor_numel": (C.c_int64, [_P, C.c_char_p]),
    "dtk_vit_encode": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "dtk_prefill": (C.c_int, [_P, _P, C.c_int, _P, C.c_uint64, C.c_int, _P]),
    "dtk_set_sampling": (C.c_int, [_P, C.POINTER(DtkSampling)]),
    "dtk_decode_launch": (C.c_int, [_P]),
    "dtk_decode_wait": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "dtk_decode": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "dtk_get_logits": (C.c_int, [_P, _P]),
    "dtk_context_len": (C.c_int, [_P]),
    "dtk_set_graph_mode": (C.c_int, [_P, C.c_int]),
    "dtk_synchronize": (C.c_int, [_P]),
    "dtk_get_stats": (C.c_int, [_P, C.POINTER(DtkStats)]),
    "dtk_num_slots": (C.c_int, [_P]),
    "dtk_max_decode_slots": (C.c_int, [_P]),
    "dtk_max_positions": (C.c_int, [_P]),
    "dtk_engine_create": (C.c_int, [_P, C.POINTER(_P)]),
    "dtk_engine_create_ops": (C.c_int, [C.POINTER(DtkEngineOps), C.POINTER(_P)]),
    "dtk_engine_destroy": (None, [_P]),
    "dtk_engine_last_error": (C.c_char_p, [_P]),
    "dtk_engine_set_flush_tokens": (C.c_int, [_P, C.POINTER(C.c_int64), C.c_int]),
    "dtk_engine_set_option": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "dtk_engine_expect": (C.c_int, [_P, C.c_int, C.c_int]),
    "dtk_engine_join": (C.c_int, [_P, C.POINTER(DtkJoin)]),
    "dtk_engine_submit": (C.c_int, [_P, C.POINTER(DtkJoin), C.POINTER(C.c_uint64)]),
    "dtk_engine_await": (C.c_int, [_P, C.c_uint64]),
    "dtk_engine_read": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]),
    "dtk_engine_leave": (C.c_int, [_P, C.c_int]),
    "dtk_engine_get_stats": (C.c_int, [_P, C.POINTER(DtkEngineStats)]),
    # ABI 7, additive: text-conditioned joins of the native run loop
    "dtk_engine_submit_text": (C.c_int, [_P, C.POINTER(DtkJoin), C.POINTER(C.c_int64), C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]),
    "dtk_engine_set_prefill_text_op": (C.c_int, [_P, DtkEngineOps.PREFILL_TEXT]),
    "dtk_prefill_slot": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_uint64, C.c_int, _P]),
    "dtk_set_sampling_slot": (C.c_int, [_P, C.c_int, C.POINTER(DtkSampling)]),
    "dtk_decode_batch_launch": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "dtk_decode_batch_wait": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "dtk_kv_fork": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "dtk_get_logits_slot": (C.c_int, [_P, C.c_int, _P]),
    "dtk_context_len_slot": (C.c_int, [_P, C.c_int]),
    "dtk_slot_lcp": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_uint64, C.POINTER(C.c_int)]),
    "dtk_slot_cached_ids": (C.c_int, [_P, C.c_int, _P, C.c_int]),
    "dtk_resume_slot": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_uint64]),
    "dtk_bench_gemv": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "dtk_set_gemv_variant": (C.c_int, [_P, C.c_int, C.c_int]),
    "dtk_set_option": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "dtk_op_gemm": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dtk_adapter_create": (C.c_int, [_P, C.POINTER(DtkAdapterConfig)]),
    "dtk_adapter_destroy": (C.c_int, [_P]),
    "dtk_has_adapter": (C.c_int, [_P]),
    "dtk_vit_encode_text": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_uint64, _P, _P]),
    "dtk_prefill_text": (C.c_int, [_P, _P, C.c_int, _P, C.c_uint64, _P, C.c_int, C.c_uint64, C.c_int, _P]),
    "dtk_prefill_slot_text": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_uint64, _P, C.c_int, C.c_uint64, C.c_int, _P]),
    "dtk_adapter_embed": (C.c_int, [_P, _P, C.c_int, _P]),
    "dtk_text_image_key": (C.c_uint64, [C.c_uint64, C.c_uint64]),
    "dtk_op_gemm_gated": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    # additive (ABI stays 7): teacher-forced scoring — log-probabilities of a given program in one pass
    "dtk_score": (C.c_int, [_P, _P, C.c_int, _P, C.c_uint64, C.c_uint32, C.c_int, _P, _P, _P]),
    "dtk_score_text": (C.c_int, [_P, _P, C.c_int, _P, C.c_uint64, _P, C.c_int, C.c_uint64, C.c_uint32, C.c_int, _P, _P, _P]),
    "dtk_op_score": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    # additive (ABI stays 7): N candidates of one prompt scored in one packed pass
    "dtk_score_packed": (C.c_int, [_P, _P, C.c_int, _P, C.c_uint64, C.c_uint32, _P, _P, C.c_int, _P, _P, _P]),
    "dtk_score_packed_text": (C.c_int, [_P, _P, C.c_int, _P, C.c_uint64, _P, C.c_int, C.c_uint64, C.c_uint32, _P, _P, C.c_int, _P, _P, _P]),
    "dtk_op_attention_seg": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    # additive (ABI stays 7): the decode attention kernels alone, single sequence and batched
    "dtk_op_attn_decode": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     _P, _P, _P, _P]),
    "dtk_op_attn_decode_b": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    # additive (ABI stays 7): kv_format "mxfp8" — the boundary, the diagnostic read, and the attention op on shadow planes
    "dtk_kv8_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    "dtk_read_kv8": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "dtk_op_attn_decode_b8": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    # additive (ABI stays 7): the weight kernels of the batched decode step alone
    "dtk_op_gemv_b": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, _P, C.c_float, _P, _P, C.c_int,
                                C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dtk_op_gemv_bkp": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P, _P, C.c_int, _P, C.c_float, _P, _P, _P, _P]),
    # additive (ABI stays 7): one role of the single-sequence decode GEMV family (prologue, epilogue, variant, weight format)
    "dtk_op_gemv_role": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P] + [C.c_int] * 9 + [C.c_float, _P, _P, _P, _P,
                                   C.c_int, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P]),
    # additive (ABI stays 7): the prefill's row kernels and attention layouts alone
    "dtk_op_rope_scatter": (C.c_int, [_P, C.c_int, _P, _P] + [C.c_int] * 8 + [_P, C.c_int, _P, _P, C.c_int, _P, _P, _P]),
    "dtk_op_rows_norm": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P] + [C.c_int] * 7 + [C.c_float, C.c_int, _P, _P]),
    "dtk_op_swiglu": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dtk_op_attention_ex": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P] + [C.c_int] * 9),
    "dtk_op_rows_move": (C.c_int, [_P, C.c_int, _P, _P, _P] + [C.c_int] * 8 + [_P]),
    # additive (ABI stays 7): one prefill GEMM launch as the product makes it (strides, offsets, in place) + the launchers' kernel record
    "dtk_op_gemm_ex": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64] + [C.c_int] * 12 + [_P]),
    "dtk_gemm_last_kernel": (C.c_int, []),
    # additive (ABI stays 7): one role of the multi-vector decode GEMV family (prologue, epilogue, nb slots, block shape)
    "dtk_op_gemv_mv_role": (C.c_int, [_P] + [C.c_int] * 4 + [_P, _P, _P] + [C.c_int] * 7 + [_P, _P, C.c_int, C.c_int, _P, _P, C.c_float,
                                      _P, _P, C.c_int, _P, _P, _P, _P, _P]),
    # additive (ABI stays 7): 13-bit planes of bf16 weight rows (csrc/w13.h): the host packer for the CPU tests, the op's packing outcome
    "dtk_w13_row_bytes": (C.c_int, [C.c_int]),
    "dtk_w13_pack_host": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P]),
    "dtk_w13_unpack_host": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "dtk_w13_op_bad_rows": (C.c_int, [_P]),
    "dtk_w13_row_bytes_host": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "dtk_w13_flagged_rows": (C.c_int, [_P, C.c_int]),
    "dtk_op_gemv": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P]),
    "dtk_op_gemv_mv": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P]),
    # additive (ABI stays 7): dtk_op_gemv on MXFP4 weights (the loader's quantiser + the decode kernel); last = de-quantised W or NULL
    "dtk_op_gemv_q4": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P]),
    "dtk_mx_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P]),
    "dtk_op_gemv_mx": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "dtk_op_attention": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dtk_op_layernorm": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_float, _P]),
    "dtk_op_sample": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int64), _P]),
    # additive (ABI stays 7): log-probabilities of sampled tokens (dtk_set_option "logprobs")
    "dtk_decode_wait_lp": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_float)]),
    "dtk_decode_batch_wait_lp": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "dtk_engine_read_lp": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int,
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]),
    "dtk_engine_set_wait_lp_op": (C.c_int, [_P, DtkEngineOps.WAIT_LP]),
    "dtk_op_sample_lp": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int64), _P, C.POINTER(C.c_float)]),
    # additive (ABI stays 7): the k <= DTK_MAX_TOP most likely tokens of every scored / sampled position
    "dtk_score_top": (C.c_int, [_P, _P, C.c_int, _P, C.c_uint64, C.c_uint32, C.c_int, _P, _P, _P, C.c_int, _P, _P]),
    "dtk_score_top_text": (C.c_int, [_P, _P, C.c_int, _P, C.c_uint64, _P, C.c_int, C.c_uint64, C.c_uint32, C.c_int, _P, _P, _P,
                                     C.c_int, _P, _P]),
    "dtk_score_packed_top": (C.c_int, [_P, _P, C.c_int, _P, C.c_uint64, C.c_uint32, _P, _P, C.c_int, _P, _P, _P, C.c_int, _P, _P]),
    "dtk_score_packed_top_text": (C.c_int, [_P, _P, C.c_int, _P, C.c_uint64, _P, C.c_int, C.c_uint64, C.c_uint32, _P, _P, C.c_int,
                                            _P, _P, _P, C.c_int, _P, _P]),
    "dtk_op_score_top": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, _P, _P, _P]),
    "dtk_decode_wait_top": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "dtk_decode_batch_wait_top": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                            C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    # additive (ABI stays 7): the records in the batch engines, and the selection kernels on host rows
    "dtk_engine_read_top": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]),
    "dtk_engine_set_wait_top_op": (C.c_int, [_P, DtkEngineOps.WAIT_TOP]),
    "dtk_op_top_logits": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    # additive (ABI stays 7): min_p / epsilon_cutoff behind top-p
    "dtk_set_sampling_ext": (C.c_int, [_P, C.POINTER(DtkSamplingExt)]),
    "dtk_set_sampling_slot_ext": (C.c_int, [_P, C.c_int, C.POINTER(DtkSamplingExt)]),
    "dtk_op_sample_ext": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int64), _P, C.POINTER(C.c_float), C.POINTER(DtkSamplingExt)]),
    "dtk_engine_submit_ext": (C.c_int, [_P, C.POINTER(DtkJoin), C.POINTER(DtkSamplingExt), C.POINTER(C.c_int64), C.c_int, C.c_uint64,
                                        C.POINTER(C.c_uint64)]),
    "dtk_engine_set_sampling_ext_op": (C.c_int, [_P, DtkEngineOps.SAMPLING_EXT]),
    # additive (ABI stays 7): presence / frequency penalty in front of the sampler chain
    "dtk_set_penalties": (C.c_int, [_P, C.c_float, C.c_float, C.c_int]),
    "dtk_set_penalties_slot": (C.c_int, [_P, C.c_int, C.c_float, C.c_float, C.c_int]),
    "dtk_op_sample_pen": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int64), _P, C.POINTER(C.c_float), C.POINTER(DtkSamplingExt),
                                    C.c_float, C.c_float, C.POINTER(C.c_int64), C.c_int]),
    "dtk_token_counts": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint16), C.c_int]),
    "dtk_engine_submit_pen": (C.c_int, [_P, C.POINTER(DtkJoin), C.POINTER(DtkSamplingExt), C.c_float, C.c_float, C.c_int,
                                        C.POINTER(C.c_int64), C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]),
    "dtk_engine_set_penalties_op": (C.c_int, [_P, DtkEngineOps.PENALTIES]),
    # additive (ABI stays 7): DRY, the penalty on verbatim repetitions, behind the presence / frequency pair
    "dtk_set_dry": (C.c_int, [_P, C.POINTER(DtkDry)]),
    "dtk_set_dry_slot": (C.c_int, [_P, C.c_int, C.POINTER(DtkDry)]),
    "dtk_dry_history": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "dtk_dry_state_bytes": (C.c_int64, [_P]),
    "dtk_op_dry_scan": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(DtkDry),
                                  C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_int]),
    "dtk_op_sample_dry": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int64), _P, C.POINTER(C.c_float), C.POINTER(DtkSamplingExt),
                                    C.c_float, C.c_float, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(DtkDry)]),
    "dtk_engine_submit_dry": (C.c_int, [_P, C.POINTER(DtkJoin), C.POINTER(DtkSamplingExt), C.c_float, C.c_float, C.c_int, C.POINTER(DtkDry),
                                        C.POINTER(C.c_int64), C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]),
    "dtk_engine_set_dry_op": (C.c_int, [_P, DtkEngineOps.DRY]),
    # additive (ABI stays 7): min_new_tokens, the EOS length decay and the logit bias, around the penalties
    "dtk_set_length_control": (C.c_int, [_P, C.POINTER(DtkLengthCtl)]),
    "dtk_set_length_control_slot": (C.c_int, [_P, C.c_int, C.POINTER(DtkLengthCtl)]),
    "dtk_set_logit_bias": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int]),
    "dtk_set_logit_bias_slot": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int]),
    "dtk_logit_bias_table": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.c_int]),
    "dtk_op_sample_shape": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int64), _P, C.POINTER(C.c_float), C.POINTER(DtkSamplingExt),
                                      C.c_float, C.c_float, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(DtkDry),
                                      C.c_int, C.POINTER(DtkLengthCtl), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int]),
    "dtk_engine_submit_shape": (C.c_int, [_P, C.POINTER(DtkJoin), C.POINTER(DtkSamplingExt), C.c_float, C.c_float, C.c_int, C.POINTER(DtkDry),
                                          C.POINTER(DtkLengthCtl), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int,
                                          C.POINTER(C.c_int64), C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]),
    "dtk_engine_set_length_control_op": (C.c_int, [_P, DtkEngineOps.LENGTH_CTL]),
    "dtk_engine_set_logit_bias_op": (C.c_int, [_P, DtkEngineOps.LOGIT_BIAS]),
    # classifier-free guidance: pairs of batch slots
    "dtk_set_guidance": (C.c_int, [_P, C.c_int, C.c_int, C.c_float]),
    "dtk_get_guidance": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "dtk_op_cfg_mix": (C.c_int, [_P, _P, _P, C.c_int, C.c_float, _P, C.POINTER(C.c_float)]),
    "dtk_bench_cfg": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float)]),
    "dtk_reserve_guidance": (C.c_int, [_P, C.c_int]),
    "dtk_batch_graph_captures": (C.c_int64, [_P]),
    "dtk_engine_submit_guided": (C.c_int, [_P, C.POINTER(DtkGuided), C.POINTER(DtkSamplingExt), C.c_float, C.c_float, C.c_int, C.POINTER(DtkDry),
                                           C.POINTER(DtkLengthCtl), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int,
                                           C.POINTER(C.c_int64), C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]),
    "dtk_engine_set_guidance_op": (C.c_int, [_P, DtkEngineOps.GUIDANCE]),
    # prompt-lookup speculative decoding of slot 0 in the multi-vector step
    "dtk_spec_begin": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "dtk_spec_set_drafts": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int]),
    "dtk_spec_launch": (C.c_int, [_P]),
    "dtk_spec_wait": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "dtk_spec_end": (C.c_int, [_P, C.c_int]),
    "dtk_bench_spec": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float)]),
    "dtk_op_spec_lookup": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int)]),
    # ... and its second draft source, a corpus of earlier programs (CORPUS_SYMBOLS: a library without them loads, and speculates
    # without a corpus)
    "dtk_spec_set_corpus": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int]),
    "dtk_spec_corpus_len": (C.c_int, [_P]),
    "dtk_spec_counters": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "dtk_op_spec_lookup_corpus": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
}
DTK_SPEC_LOOKUP, DTK_SPEC_TABLE, DTK_SPEC_MAX_NGRAM = 0, 1, 16
DTK_SPEC_CORPUS_MAX = 65536
DTK_SPEC_FROM_NONE, DTK_SPEC_FROM_HISTORY, DTK_SPEC_FROM_CORPUS = 0, 1, 2
CORPUS_SYMBOLS = ("dtk_spec_set_corpus", "dtk_spec_corpus_len", "dtk_spec_counters", "dtk_op_spec_lookup_corpus")


def corpus_call(lib, name: str):
    """the corpus entry point `name` of lib, or a DtkError that says what is missing: only a call that uses a corpus needs them"""
    fn = getattr(lib, name, None)
    if fn is None:
        raise DtkError(f"{name} is missing: this library has no prompt-lookup corpus (prompt_lookup_corpus needs a build of this tree)")
    return fn

_lib = None


class DtkError(RuntimeError):
    pass


def load_library() -> C.CDLL:
    """Load libdtk_hip.so once.  If torch is importable it is imported FIRST so that exactly one
    HIP runtime (torch's bundled libamdhip64.so.7) is in the process — the library's NEEDED
    libamdhip64.so.7 then resolves to the already-loaded copy and torch.distributed (RCCL) can
    share the process.  DTK_HIP_RUNTIME=system skips that and uses /opt/rocm via RUNPATH."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise DtkError(
            f"{LIB_PATH} is missing: build it with ./build.sh (hipcc --offload-arch=gfx950). "
            "detikzify_amd has no CPU fallback.")
    if os.environ.get("DTK_HIP_RUNTIME", "torch") != "system":
        try:
            import torch  # noqa: F401  (side effect: loads torch/lib/libamdhip64.so)
        except Exception:  # pragma: no cover - torch-less deployments use the system runtime
            pass
    lib = C.CDLL(str(LIB_PATH), mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        if name in CORPUS_SYMBOLS and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError here = ABI mismatch, loud by design
        fn.restype, fn.argtypes = res, args
    if lib.dtk_abi_version() != DTK_ABI_VERSION:
        raise DtkError(f"ABI version {lib.dtk_abi_version()} != {DTK_ABI_VERSION}")
    for which, (struct, field) in enumerate(((DtkConfig, None), (DtkSampling, None), (DtkStats, None), (DtkSampling, "seed"),
                                             (DtkConfig, "reserved"), (DtkStats, "probe_event_pair_ms"))):
        ours = C.sizeof(struct) if field is None else getattr(struct, field).offset
        if lib.dtk_abi_struct_size(which) != ours:     # a drifted struct would corrupt every call: refuse to run
            raise DtkError(f"struct layout mismatch with include/dtk.h: {struct.__name__}{'.' + field if field else ''} "
                           f"is {ours} here, {lib.dtk_abi_struct_size(which)} in the library")
    if lib.dtk_abi_struct_size(11) != C.sizeof(DtkAdapterConfig):
        raise DtkError(f"struct layout mismatch with include/dtk.h: DtkAdapterConfig is {C.sizeof(DtkAdapterConfig)} here, "
                       f"{lib.dtk_abi_struct_size(11)} in the library")
    if lib.dtk_abi_struct_size(12) != C.sizeof(DtkSamplingExt):
        raise DtkError(f"struct layout mismatch with include/dtk.h: DtkSamplingExt is {C.sizeof(DtkSamplingExt)} here, "
                       f"{lib.dtk_abi_struct_size(12)} in the library")
    if lib.dtk_abi_struct_size(14) != C.sizeof(DtkDry):
        raise DtkError(f"struct layout mismatch with include/dtk.h: DtkDry is {C.sizeof(DtkDry)} here, "
                       f"{lib.dtk_abi_struct_size(14)} in the library")
    if lib.dtk_abi_struct_size(16) != C.sizeof(DtkLengthCtl):
        raise DtkError(f"struct layout mismatch with include/dtk.h: DtkLengthCtl is {C.sizeof(DtkLengthCtl)} here, "
                       f"{lib.dtk_abi_struct_size(16)} in the library")
    _lib = lib
    return lib


def check(lib, ctx, rc: int, what: str):
    if rc != 0:
        msg = lib.dtk_last_error(ctx)
        text = msg.decode(errors="replace") if msg else ""
        if rc == -1 and ("image patch tokens" in text):
            raise ValueError(text)          # same exception type/message as the reference
        raise DtkError(f"{what} failed ({rc}): {text}")
