#!/usr/bin/env python
"""What top-k alternatives cost: in ONE process, the settings alternating,
  * the packed scoring pass, 16 candidates x 200 tokens, top_logprobs = 0, 1, 8: device ms (the library's HIP events);
  * single-sequence sampled decode with "logprobs" on, "top_logprobs" = 0 and 8: tokens/s;
  * the 64-slot batched step (slots forked from one prompt), the same two settings: ms per step;
  * both of these under "top_kernel" 0 (the library's own rule: the keys without a kernel in their name), 1 (k_top_logits, one block
    per sequence) and 2 (k_top_slice + k_top_merge);
  * 64 sequences in the native batch engine, built without and with top_logprobs=8 (log-probabilities on in both): steps/s.
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
    ap.add_argument("--engine-tokens", type=int, default=256, help="tokens per sequence of the engine leg (0 = skip it)")
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
    res["vocab"] = int(cfg.vocab)

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

    def engine64(k):
        """64 text-only sequences of one prompt in the native engine, sampled, args.engine_tokens each -> steps/s between the first launch
        and the last collect"""
        import threading
        from detikzify_amd.infer.engine import NativeBatchEngine
        eng = NativeBatchEngine(model, max_batch=64, gather=64, gather_timeout=30.0, **({"top_logprobs": k} if k else {}))
        errs = []

        def run(s):
            try:
                emit = lambda tok: False
                emit.many = lambda toks: False
                with eng.sequence(ids, None, {**samp, "seed": 100 + s}, max_new_tokens=args.engine_tokens, stop_ids=(), per_token=False,
                                  logprobs=True, **({"top_logprobs": k} if k else {})) as seq:
                    seq.run(emit)
            except BaseException as e:  # noqa: BLE001
                errs.append(e)
        try:
            ths = [threading.Thread(target=run, args=(s,)) for s in range(64)]
            [t.start() for t in ths]
            [t.join() for t in ths]
            st = eng.native_stats()        # (the unrounded stamps: stats() rounds the span to a millisecond)
        finally:
            eng.close()
        if errs:
            raise errs[0]
        return st["steps"] / (st["last_collect_t"] - st["first_launch_t"])

    model.enable_logprobs()
    med = statistics.median
    for kern in (0, 1, 2):       # 0: whatever top_logits_launch's own rule selects (the keys without a kernel in their name)
        model.set_option("top_kernel", kern)
        tag = f"_kernel{kern}" if kern else ""
        res["single_tok_s" + tag] = {"0": [], "8": []}
        res["batch64_step_ms" + tag] = {"0": [], "8": []}
        for _ in range(args.rounds):
            for k in (0, 8):
                res["single_tok_s" + tag][str(k)].append(round(single(k), 2))
        for _ in range(args.rounds):
            for k in (0, 8):
                res["batch64_step_ms" + tag][str(k)].append(round(batch64(k), 4))
        if kern:
            res["single_k8_over_k0" + tag] = round(med(res["single_tok_s" + tag]["8"]) / med(res["single_tok_s" + tag]["0"]), 5)
            res["batch64_k8_over_k0" + tag] = round(med(res["batch64_step_ms" + tag]["8"]) / med(res["batch64_step_ms" + tag]["0"]), 5)
    model.set_option("top_kernel", 0)
    model.enable_top_logprobs(0)
    if args.engine_tokens > 0:
        res["engine64_steps_s"] = {"0": [], "8": []}
        engine64(0)                                  # warm-up: the graphs of the 64-slot step
        for _ in range(args.rounds):
            for k in (0, 8):
                res["engine64_steps_s"][str(k)].append(round(engine64(k), 3))
        res["engine64_k8_over_k0"] = round(med(res["engine64_steps_s"]["8"]) / med(res["engine64_steps_s"]["0"]), 5)
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
