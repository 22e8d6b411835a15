#!/usr/bin/env python
"""What DRY costs: in ONE process, off (the sampler kernels as they were) against dry_multiplier = 0.8, dry_base = 1.75,
dry_allowed_length = 2 with the history starting at position 0 (k_dry_scan + the PN instantiations + the trailing kernel), alternating,
  * single-sequence sampled decode: tokens/s;
  * the 64-slot batched step (slots forked from one prompt, the prefix context): ms per step.
v1 models (<= 32 768 tokens) run k_sample_fast, v2 models the multi-block chain.  Synthetic weights, real shapes.
Writes profiles/dry_<model>.json."""
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

ON = dict(multiplier=0.8, base=1.75, allowed_length=2, start=0)


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
    samp = dict(do_sample=True, temperature=0.8, top_p=0.95, seed=7, bad_ids=[cfg.image_token_id])
    res = {"model": args.model, "vocab": int(cfg.vocab), "prompt_tokens": int(ids.numel()), "on": ON,
           "single_tok_s": {"off": [], "on": []}, "batch64_step_ms": {"off": [], "on": []}}

    def single(dry):
        model.set_sampling(**samp)
        if dry:
            model.set_dry(**dry)
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

    def batch64(dry):
        model.set_sampling(do_sample=False, slot=64)
        model.prefill(ids, None, slot=64)
        for s in range(64):
            model.set_sampling(slot=s, **{**samp, "seed": 100 + s})
            if dry:
                model.set_dry(slot=s, **dry)
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
        for tag, dry in (("off", {}), ("on", ON)):
            res["single_tok_s"][tag].append(round(single(dry), 2))
    for _ in range(args.rounds):
        for tag, dry in (("off", {}), ("on", ON)):
            res["batch64_step_ms"][tag].append(round(batch64(dry), 4))
    med = statistics.median
    res["single_on_over_off"] = round(med(res["single_tok_s"]["on"]) / med(res["single_tok_s"]["off"]), 5)
    res["batch64_on_over_off"] = round(med(res["batch64_step_ms"]["on"]) / med(res["batch64_step_ms"]["off"]), 5)
    out = Path(args.out) if args.out else ROOT / "profiles" / f"dry_{args.model.replace('detikzify-', '')}.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    if out.exists():       # the comparisons against the parent commit (bench.py and bench_penalty.py runs) live in the same file
        try:
            before = json.loads(out.read_text())
        except ValueError:
            before = {}
        for key in ("off_path_vs_parent", "penalties_only_vs_parent"):
            if key in before:
                res[key] = before[key]
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
