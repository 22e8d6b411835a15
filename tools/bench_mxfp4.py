#!/usr/bin/env python
"""What MXFP4 decoder weights buy at B = 1 (DESIGN 3.1c'): in ONE process, three contexts of one model (weight_format bf16, fp8,
mxfp4; synthetic weights, real shapes) alternating --rounds times,
  * greedy single-sequence decode of bench.py's rollout (one image, --new-tokens tokens): tokens/s of the decode part
    (rollout seconds - the prefill's device ms), and that as bytes/s (weights once + the mean context's KV) against 8 TB/s;
  * every weight kernel of the step — q/k/v, o_proj, gate/up (the dominant one), down, lm_head — on its own, back to back over
    all layers' weights between one pair of HIP events on the library's stream (dtk_bench_gemv, the format's own kernel), as
    microseconds and as bytes/s against 8 TB/s; the step minus their sum = attention + sampler + launch boundaries.
Writes profiles/mxfp4_<model>.json."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

HBM_PEAK = 8e12
ROLES = ["qkv", "o_proj", "gate_up", "down", "lm_head"]
FORMATS = ["bf16", "fp8", "mxfp4"]


def role_bytes(cfg, fmt):
    """weight bytes one launch of each role streams (norm vectors and x left out: < 0.1 %)"""
    d, ff, V = cfg.hidden, cfg.ffn, cfg.vocab
    kvd = cfg.num_kv_heads * cfg.head_dim
    shapes = {"qkv": (d + 2 * kvd, d), "o_proj": (d, d), "gate_up": (2 * ff, d), "down": (d, ff), "lm_head": (V, d)}
    out = {}
    for r, (N, K) in shapes.items():
        f = "fp8" if (fmt == "mxfp4" and r == "lm_head") else fmt
        out[r] = {"bf16": 2 * N * K, "fp8": N * K + 4 * N, "mxfp4": N * ((K + 31) // 32) * 17}[f]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="detikzify-ds-7b")
    ap.add_argument("--new-tokens", type=int, default=512, help="bench.py's rollout length")
    ap.add_argument("--rounds", type=int, default=3, help="alternations")
    ap.add_argument("--chain-reps", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import detikzify_amd.model as dmodel
    from detikzify_amd.util import expand
    from detikzify_amd.util.synthetic import sketch_image

    models = {}
    for f in FORMATS:
        models[f], proc = dmodel.load(args.model, synthetic=1234, weight_format=f)
    cfg = models["bf16"].config
    img = sketch_image(0, 224)
    enc = proc(images=expand(img, max(img.size), do_trim=True), return_tensors="pt")
    ids, px = enc.input_ids, enc.pixel_values
    T0, n_new = ids.shape[1], args.new_tokens
    eos = cfg.eos_token_id if isinstance(cfg.eos_token_id, (list, tuple)) else [cfg.eos_token_id]
    kw = dict(pixel_values=px, bad_words_ids=[[cfg.image_token_id]], begin_suppress_tokens=list(eos), suppress_tokens=list(eos),
              max_new_tokens=n_new, eos_token_id=-1, do_sample=False)

    def rollout(m):
        t0 = time.perf_counter()
        out = m.generate(input_ids=ids, **kw)
        dt = time.perf_counter() - t0
        assert out.shape[1] == T0 + n_new
        return n_new / (dt - m.stats()["last_prefill_ms"] / 1e3)

    def chain(m, role):
        us = C.c_float(0.0)
        m._check(m.lib.dtk_bench_gemv(m._ctx, role, 0xFF | 0x800, args.chain_reps, C.byref(us)), "dtk_bench_gemv")
        return float(us.value)

    res = {"model": args.model, "prefix_tokens": int(T0), "new_tokens": n_new, "layers": cfg.layers, "hbm_peak_bytes_per_s": HBM_PEAK,
           "decode_tok_s": {f: [] for f in FORMATS}, "kernel_us": {f: {r: [] for r in ROLES} for f in FORMATS}}
    for f in FORMATS:
        rollout(models[f])                    # warm-up: code objects, the graph capture, the quantiser
    for _ in range(args.rounds):
        for f in FORMATS:
            res["decode_tok_s"][f].append(round(rollout(models[f]), 2))
    for _ in range(args.rounds):
        for f in FORMATS:
            for i, r in enumerate(ROLES):
                res["kernel_us"][f][r].append(round(chain(models[f], i), 3))
    med = statistics.median
    summ = {}
    for f in FORMATS:
        st = models[f].stats()
        W, Kb = st["weight_bytes_per_token"], st["kv_bytes_per_ctx_token"]
        bytes_tok = W + Kb * (T0 + (n_new - 1) / 2.0)
        tok_s = med(res["decode_tok_s"][f])
        rb = role_bytes(cfg, f)
        ker = {r: med(res["kernel_us"][f][r]) for r in ROLES}
        gemv_us = cfg.layers * sum(ker[r] for r in ROLES[:4]) + ker["lm_head"]
        step_us = 1e6 / tok_s
        summ[f] = {"decode_tok_s": tok_s, "step_us": round(step_us, 2), "weight_bytes_per_token": int(W), "bytes_per_token": int(bytes_tok),
                   "step_frac_of_hbm_peak": round(bytes_tok * tok_s / HBM_PEAK, 4),
                   "kernel_us": ker, "kernel_bytes": rb,
                   "kernel_frac_of_hbm_peak": {r: round(rb[r] / (ker[r] * 1e-6) / HBM_PEAK, 4) for r in ROLES},
                   "dominant_kernel": "gate_up", "weight_kernels_us_per_step": round(gemv_us, 2),
                   "rest_us_per_step": round(step_us - gemv_us, 2)}      # attention, sampler, launch boundaries inside the graph
    res["summary"] = summ
    res["mxfp4_over_fp8"] = round(summ["mxfp4"]["decode_tok_s"] / summ["fp8"]["decode_tok_s"], 4)
    res["mxfp4_over_bf16"] = round(summ["mxfp4"]["decode_tok_s"] / summ["bf16"]["decode_tok_s"], 4)
    res["fp8_over_bf16"] = round(summ["fp8"]["decode_tok_s"] / summ["bf16"]["decode_tok_s"], 4)
    out = Path(args.out) if args.out else ROOT / "profiles" / f"mxfp4_{args.model.replace('detikzify-', '')}.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
