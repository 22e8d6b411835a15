#!/usr/bin/env python
"""What min_new_tokens / exponential_decay_length_penalty / logit_bias cost: in ONE process, off (the sampler kernels as
they were) against
  * "length": min_new_tokens and a decay on one EOS id (the PN instantiations with a length record; both thresholds are crossed
    during the timed steps), and
  * "length+bias": the same with a 256-entry bias table (one more float read beside every logit), and, from the same run,
  * "penalties": (presence, frequency) = (0.6, 0.4), the PN instantiations' own on-cost,
alternating,
  * single-sequence sampled decode: tokens/s;
  * the 64-slot batched step (slots forked from one prompt, the prefix context): ms per step.
v1 models (<= 32 768 tokens) run k_sample_fast, v2 models the multi-block chain.  Synthetic weights, real shapes.
Writes profiles/length_<model>.json."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

LEGS = ("off", "length", "length+bias", "penalties")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="detikzify-ds-7b")
    ap.add_argument("--prompt", type=int, default=300, help="prompt tokens (text only)")
    ap.add_argument("--tokens", type=int, default=256, help="timed decode steps of the single-sequence leg")
    ap.add_argument("--steps", type=int, default=64, help="timed steps of the 64-slot leg")
    ap.add_argument("--rounds", type=int, default=3, help="alternations")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from detikzify_amd.model import load
    model, _ = load(args.model, synthetic=1234, max_positions=3584, batch_slots=65)
    cfg = model.config
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab - 1, (args.prompt + 8,), generator=g)
    ids = ids[ids != cfg.image_token_id][:args.prompt].contiguous()
    T = int(ids.numel())
    samp = dict(do_sample=True, temperature=0.8, top_p=0.95, seed=7, bad_ids=[cfg.image_token_id])
    eos = (int(cfg.vocab) - 1,)
    # the minimum ends and the decay starts inside the timed steps; a factor this close to 1 leaves the EOS logit where it is
    length = dict(min_new_tokens=16, decay=(24, 1.0001), start=T, eos_ids=eos)
    bias = {3 + 97 * i: (0.25 if i % 2 else -0.25) for i in range(256)}
    res = {"model": args.model, "vocab": int(cfg.vocab), "prompt_tokens": T,
           "length": {"min_new_tokens": 16, "decay": [24, 1.0001]}, "bias_entries": len(bias), "penalties": {"presence": 0.6, "frequency": 0.4},
           "single_tok_s": {k: [] for k in LEGS}, "batch64_step_ms": {k: [] for k in LEGS}}

    def apply(leg, slot=None):
        if leg in ("length", "length+bias"):
            model.set_length_control(slot=slot, **length)
        if leg == "length+bias":
            model.set_logit_bias(bias, slot=slot)
        if leg == "penalties":
            model.set_penalties(0.6, 0.4, 0, slot=slot)

    def single(leg):
        model.set_sampling(**samp)
        apply(leg)
        model.prefill(ids, None)
        for _ in range(8):
            model.decode_launch(); model.decode_wait()
        model.decode_launch()
        t0 = time.perf_counter()
        for _ in range(args.tokens):       # one step always in flight, as generate() keeps it
            model.decode_launch(); model.decode_wait()
        dt = time.perf_counter() - t0
        model.decode_wait()
        return args.tokens / dt

    def batch64(leg):
        model.set_sampling(do_sample=False, slot=64)
        model.prefill(ids, None, slot=64)
        for s in range(64):
            model.set_sampling(slot=s, **{**samp, "seed": 100 + s})
            apply(leg, slot=s)
            model.kv_fork(64, s, ids.numel())
        for _ in range(8):
            model.decode_batch_launch(range(64)); model.decode_batch_wait()
        model.decode_batch_launch(range(64))
        t0 = time.perf_counter()
        for _ in range(args.steps):
            model.decode_batch_launch(range(64)); model.decode_batch_wait()
        dt = time.perf_counter() - t0
        model.decode_batch_wait()
        return 1e3 * dt / args.steps

    for _ in range(args.rounds):
        for leg in LEGS:
            res["single_tok_s"][leg].append(round(single(leg), 2))
    for _ in range(args.rounds):
        for leg in LEGS:
            res["batch64_step_ms"][leg].append(round(batch64(leg), 4))
    med = statistics.median
    for leg in LEGS[1:]:
        res[f"single_{leg}_over_off"] = round(med(res["single_tok_s"][leg]) / med(res["single_tok_s"]["off"]), 5)
        res[f"batch64_{leg}_over_off"] = round(med(res["batch64_step_ms"][leg]) / med(res["batch64_step_ms"]["off"]), 5)
    out = Path(args.out) if args.out else ROOT / "profiles" / f"length_{args.model.replace('detikzify-', '')}.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    if out.exists():       # the off-path comparison against the parent commit (bench.py runs) lives in the same file
        try:
            kept = json.loads(out.read_text()).get("off_path_vs_parent")
        except ValueError:
            kept = None
        if kept is not None:
            res["off_path_vs_parent"] = kept
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
