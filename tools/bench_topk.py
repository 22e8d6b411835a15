#!/usr/bin/env python
"""What top-k alternatives cost: in ONE process, the settings alternating,
  * the packed scoring pass, 16 candidates x 200 tokens, top_logprobs = 0, 1, 8: device ms (the library's HIP events);
  * single-sequence sampled decode with "logprobs" on, "top_logprobs" = 0 and 8: tokens/s;
  * the 64-slot batched step (slots forked from one prompt), the same two settings: ms per step.
Synthetic weights, real shapes.  Writes profiles/topk_<model>.json."""
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
    cands = [torch.randint(10, 1000, (200,), generator=g) for _ in range(16)]
    res = {"model": args.model, "prompt_tokens": int(ids.numel()), "score_packed_16x200_event_ms": {"0": [], "1": [], "8": []},
           "single_tok_s": {"0": [], "8": []}, "batch64_step_ms": {"0": [], "8": []}}

    for r in range(args.rounds + 2):          # two warm-up rounds: workspaces, the prompt's cache
        for k in (0, 1, 8):
            model.score_candidates(ids, cands, None, reuse=True, **({"top_logprobs": k} if k else {}))
            if r >= 2:
                res["score_packed_16x200_event_ms"][str(k)].append(round(model.stats()["last_prefill_ms"], 3))

    def single(k):
        model.set_sampling(**samp)
        model.enable_top_logprobs(k)
        model.prefill(ids, None)
        wait = (lambda: model.decode_wait(top=True)) if k else model.decode_wait_lp
        for _ in range(8):
            model.decode_launch(); wait()
        model.decode_launch()
        t0 = time.perf_counter()
        for _ in range(args.tokens):       # one step always in flight, as generate() keeps it
            model.decode_launch(); wait()
        dt = time.perf_counter() - t0
        wait()
        return args.tokens / dt

    def batch64(k):
        model.enable_top_logprobs(k)
        model.set_sampling(do_sample=False, slot=64)
        model.prefill(ids, None, slot=64)
        for s in range(64):
            model.set_sampling(slot=s, **{**samp, "seed": 100 + s})
            model.kv_fork(64, s, ids.numel())
        wait = (lambda: model.decode_batch_wait(top=True)) if k else model.decode_batch_wait_lp
        for _ in range(8):
            model.decode_batch_launch(range(64)); wait()
        model.decode_batch_launch(range(64))
        t0 = time.perf_counter()
        for _ in range(args.steps):
            model.decode_batch_launch(range(64)); wait()
        dt = time.perf_counter() - t0
        wait()
        return 1e3 * dt / args.steps

    model.enable_logprobs()
    for _ in range(args.rounds):
        for k in (0, 8):
            res["single_tok_s"][str(k)].append(round(single(k), 2))
    for _ in range(args.rounds):
        for k in (0, 8):
            res["batch64_step_ms"][str(k)].append(round(batch64(k), 4))
    med = statistics.median
    sp = res["score_packed_16x200_event_ms"]
    res["score_k1_minus_k0_ms"] = round(med(sp["1"]) - med(sp["0"]), 3)
    res["score_k8_minus_k0_ms"] = round(med(sp["8"]) - med(sp["0"]), 3)
    res["single_k8_over_k0"] = round(med(res["single_tok_s"]["8"]) / med(res["single_tok_s"]["0"]), 5)
    res["batch64_k8_over_k0"] = round(med(res["batch64_step_ms"]["8"]) / med(res["batch64_step_ms"]["0"]), 5)
    out = Path(args.out) if args.out else ROOT / "profiles" / f"topk_{args.model.replace('detikzify-', '')}.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
