#!/usr/bin/env python
"""What dtk_set_option "logprobs" costs: in ONE process, alternating option off / on,
  * single-sequence sampled decode, tokens/s;
  * the 64-slot batched step (slots forked from one prompt), ms per step;
  * for reference, model.score of a 512-token program after the same prompt: the pass the option replaces.
Synthetic weights, real shapes.  Writes profiles/logprobs_<model>.json (+ --bench-lines: bench.py result lines recorded beside it)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="detikzify-ds-7b")
    ap.add_argument("--prompt", type=int, default=300, help="prompt tokens (text only: the prefix context of the steps)")
    ap.add_argument("--tokens", type=int, default=256, help="timed decode steps of the single-sequence leg")
    ap.add_argument("--steps", type=int, default=64, help="timed steps of the 64-slot leg")
    ap.add_argument("--rounds", type=int, default=3, help="off/on alternations")
    ap.add_argument("--bench-lines", nargs="*", default=[], metavar="TAG=FILE", help="bench.py JSON lines to record (this commit / its parent)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from detikzify_amd.model import load
    model, _ = load(args.model, synthetic=1234, max_positions=1024, batch_slots=65)
    cfg = model.config
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab - 1, (args.prompt + 8,), generator=g)
    ids = ids[ids != cfg.image_token_id][:args.prompt].contiguous()
    samp = dict(do_sample=True, temperature=0.8, top_p=0.95, seed=7, bad_ids=[cfg.image_token_id])

    def single(on):
        model.set_option("logprobs", on)
        model.set_sampling(**samp)
        model.prefill(ids, None)
        wait = model.decode_wait_lp if on else model.decode_wait
        for _ in range(8):
            model.decode_launch(); wait()
        model.decode_launch()
        t0 = time.perf_counter()
        for _ in range(args.tokens):       # one step always in flight, as generate() keeps it
            model.decode_launch(); wait()
        dt = time.perf_counter() - t0
        wait()
        return args.tokens / dt

    def batch64(on):
        model.set_option("logprobs", on)
        model.set_sampling(do_sample=False, slot=64)
        model.prefill(ids, None, slot=64)
        for s in range(64):
            model.set_sampling(slot=s, **{**samp, "seed": 100 + s})
            model.kv_fork(64, s, ids.numel())
        wait = model.decode_batch_wait_lp if on else model.decode_batch_wait
        for _ in range(8):
            model.decode_batch_launch(range(64)); wait()
        model.decode_batch_launch(range(64))
        t0 = time.perf_counter()
        for _ in range(args.steps):
            model.decode_batch_launch(range(64)); wait()
        dt = time.perf_counter() - t0
        wait()
        return 1e3 * dt / args.steps

    res = {"model": args.model, "prompt_tokens": int(ids.numel()), "single_tok_s": {"off": [], "on": []}, "batch64_step_ms": {"off": [], "on": []}}
    for _ in range(args.rounds):
        for on in (0, 1):
            res["single_tok_s"]["on" if on else "off"].append(round(single(on), 2))
    for _ in range(args.rounds):
        for on in (0, 1):
            res["batch64_step_ms"]["on" if on else "off"].append(round(batch64(on), 4))
    model.set_option("logprobs", 0)
    prog = torch.randint(3, cfg.vocab - 1, (520,), generator=g)
    prog = prog[prog != cfg.image_token_id][:512]
    full = torch.cat([ids, prog])
    times = []
    for _ in range(4):
        t0 = time.perf_counter()
        model.score(full, None, first=int(ids.numel()))
        times.append(1e3 * (time.perf_counter() - t0))
    res["score_512_ms"] = [round(t, 3) for t in times[1:]]
    med = statistics.median
    res["single_on_over_off"] = round(med(res["single_tok_s"]["on"]) / med(res["single_tok_s"]["off"]), 5)
    res["batch64_on_over_off"] = round(med(res["batch64_step_ms"]["on"]) / med(res["batch64_step_ms"]["off"]), 5)
    res["bench_lines"] = {}
    for item in args.bench_lines:
        tag, _, path = item.partition("=")
        res["bench_lines"][tag] = json.loads(Path(path).read_text().strip().splitlines()[-1])
    out = Path(args.out) if args.out else ROOT / "profiles" / f"logprobs_{args.model.replace('detikzify-', '')}.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
