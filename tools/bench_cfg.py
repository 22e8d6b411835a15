#!/usr/bin/env python
"""What classifier-free guidance costs: in ONE process, on a model loaded with batch_slots=2 (the multi-vector family),
alternating,
  * "slot":   one unguided sequence in slot 0 (a 1-vector step): decode tokens/s;
  * "pair":   two unguided sequences in slots 0 and 1 (a 2-vector step, no guidance kernels): steps/s;
  * "guided": a guided pair in slots 0 and 1 (the same 2-vector step + k_cfg_lse, k_cfg_mix, k_cfg_follow): tokens/s;
  * "single": the single-sequence path (dtk_decode_*), for reference: tokens/s;
and the guidance launches' own time per step from HIP events around back-to-back launches (dtk_bench_cfg).  The expectation to compare
against: a guided token costs about one 2-vector step plus the mixing launches, not two single-sequence steps.
Synthetic weights, real shapes.  Writes profiles/cfg_<model>.json."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

LEGS = ("slot", "pair", "guided", "single")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="detikzify-ds-7b")
    ap.add_argument("--prompt", type=int, default=300, help="prompt tokens (text only)")
    ap.add_argument("--tokens", type=int, default=192, help="timed decode steps per leg")
    ap.add_argument("--rounds", type=int, default=3, help="alternations")
    ap.add_argument("--scale", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from detikzify_amd.model import load
    model, _ = load(args.model, synthetic=1234, max_positions=2048, batch_slots=2)
    cfg = model.config
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab - 1, (args.prompt + 8,), generator=g)
    ids = ids[ids != cfg.image_token_id][:args.prompt].contiguous()
    neg = torch.cat([ids[: args.prompt // 2], ids.flip(0)[: args.prompt - args.prompt // 2]])      # the negative prompt: same length, other text
    samp = dict(do_sample=True, temperature=0.8, top_p=0.95, seed=7, bad_ids=[cfg.image_token_id])
    per = 1024 * max(1, -(-int(cfg.vocab) // (1024 * 128)))        # cfg_shape (csrc/kernels_cfg.hip): elements per slice, a function of V alone
    res = {"model": args.model, "vocab": int(cfg.vocab), "prompt_tokens": int(ids.numel()), "guidance_scale": args.scale,
           "slices": -(-int(cfg.vocab) // per), "elements_per_slice": per,
           "tok_s": {k: [] for k in LEGS}, "kernels_us_per_step": {}}

    def batch(slots, guided):
        model.set_sampling(slot=0, **samp)
        model.prefill(ids, None, slot=0)
        if 1 in slots:
            model.set_sampling(slot=1, **({} if guided else {**samp, "seed": 8}))
            model.prefill(neg, None, slot=1)
        if guided:
            model.set_guidance(args.scale, 0, 1)
        try:
            for _ in range(8):
                model.decode_batch_launch(slots); model.decode_batch_wait()
            model.decode_batch_launch(slots)
            t0 = time.perf_counter()
            for _ in range(args.tokens):       # one step always in flight, as generate() keeps it
                model.decode_batch_launch(slots); model.decode_batch_wait()
            dt = time.perf_counter() - t0
            model.decode_batch_wait()
            if guided and not res["kernels_us_per_step"]:
                us = (C.c_float * 2)()
                model._check(model.lib.dtk_bench_cfg(model._ctx, 50, us), "dtk_bench_cfg")
                res["kernels_us_per_step"] = {"k_cfg_lse+k_cfg_mix": round(float(us[0]), 3), "k_cfg_follow": round(float(us[1]), 3)}
        finally:
            if guided:
                model.set_guidance(None, 0, None)
        return args.tokens / dt

    def single():
        model.set_sampling(**samp)
        model.prefill(ids, None)
        for _ in range(8):
            model.decode_launch(); model.decode_wait()
        model.decode_launch()
        t0 = time.perf_counter()
        for _ in range(args.tokens):
            model.decode_launch(); model.decode_wait()
        dt = time.perf_counter() - t0
        model.decode_wait()
        return args.tokens / dt

    run = {"slot": lambda: batch([0], False), "pair": lambda: batch([0, 1], False), "guided": lambda: batch([0, 1], True), "single": single}
    for _ in range(args.rounds):
        for leg in LEGS:
            res["tok_s"][leg].append(round(run[leg](), 2))
    med = {k: statistics.median(v) for k, v in res["tok_s"].items()}
    step_us = {k: 1e6 / v for k, v in med.items()}
    res["median_tok_s"] = {k: round(v, 2) for k, v in med.items()}
    res["step_us"] = {k: round(v, 2) for k, v in step_us.items()}
    res["guided_over_slot_tok_s"] = round(med["guided"] / med["slot"], 5)
    res["guided_over_single_tok_s"] = round(med["guided"] / med["single"], 5)
    res["guided_minus_pair_step_us"] = round(step_us["guided"] - step_us["pair"], 2)
    kus = sum(res["kernels_us_per_step"].values())
    res["kernels_share_of_guided_step"] = round(kus / step_us["guided"], 5)
    out = Path(args.out) if args.out else ROOT / "profiles" / f"cfg_{args.model.replace('detikzify-', '')}.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
