#!/usr/bin/env python
"""What kv_format "mxfp8" buys and costs.  One process per format (two 64-slot contexts do not fit side by side; run
it A B A B: --kv-format bf16, mxfp8, bf16, mxfp8): a 65-slot context, one prefix of `--prefix` tokens prefilled into the prefix
slot, forked whole into the 64 decoding slots, which then decode to depth with sampling on — so every private row is a decoded row.
Recorded: the wall time per 64-slot step (launch to wait, pipelined two deep like the engines) in windows of `--window` steps centred
on 260 / 480 private keys and in the window of steps 1 .. 11 for "4" (a window centred on 4 would begin before the first step: it holds
the run's first steps, so its minimum is the pipeline filling — read the median).  Synthetic weights, real shapes.  Appends one JSON
line per run to --out;  `--assemble RUNS.jsonl --out profiles/kv8_<model>.json` turns the lines of one visit into the committed
profile (means of the runs' medians per format, their ratio, the bf16 runs' own spread).  The tail kernel alone is
tools/probe/kv8_tail_probe.hip."""
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

DEPTHS = (4, 260, 480)


WHAT = ("tools/bench_kv8.py: 64 forks of one 243-token prefix decode to depth (sampling on), wall ms per 64-slot step in 16-step windows centred "
        "on 260 / 480 private keys and in steps 1 .. 11 for '4' (1 to 11 private keys, not centred on 4; it contains the first steps of the run: "
        "its min is the pipeline filling, read the median); one process per format, run bf16 mxfp8 bf16 mxfp8 in one visit")


def assemble(src, dst):
    """the JSON lines of one visit -> the profile: per format the mean of the runs' medians, mxfp8 / bf16, and how far the first and the
    last bf16 run lie apart (relative to their mean)"""
    runs = [json.loads(l) for l in open(src) if l.strip()]
    depths = [str(d) for d in DEPTHS]
    med = {f: {d: statistics.mean(r["step_ms"][d]["median"] for r in runs if r["kv_format"] == f) for d in depths} for f in ("bf16", "mxfp8")}
    bf = [r for r in runs if r["kv_format"] == "bf16"]
    out = {"what": WHAT, "runs": runs, "mean_of_run_medians_ms": med,
           "ratio_mxfp8_over_bf16": {d: med["mxfp8"][d] / med["bf16"][d] for d in depths},
           "bf16_run_to_run_spread": {d: abs(bf[0]["step_ms"][d]["median"] - bf[-1]["step_ms"][d]["median"]) / med["bf16"][d] for d in depths}}
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("mean_of_run_medians_ms", "ratio_mxfp8_over_bf16", "bf16_run_to_run_spread")}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="detikzify-ds-7b")
    ap.add_argument("--weight-format", default="bf16")
    ap.add_argument("--kv-format", default="bf16")
    ap.add_argument("--prefix", type=int, default=243)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--assemble", default=None, metavar="RUNS.jsonl", help="no run: write the profile --out from the lines of one visit")
    args = ap.parse_args()
    if args.assemble:
        if not args.out:
            ap.error("--assemble needs --out")
        assemble(args.assemble, args.out)
        return
    from detikzify_amd.model import load
    model, _ = load(args.model, synthetic=1234, max_positions=1024, batch_slots=65, weight_format=args.weight_format, kv_format=args.kv_format)
    cfg = model.config
    if args.weight_format == "fp8":
        model.set_option("act_fp8", 1)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab - 1, (args.prefix + 8,), generator=g)
    ids = ids[ids != cfg.image_token_id][:args.prefix].contiguous()
    NS = model.max_decode_slots()
    slots = list(range(NS))
    model.prefill(ids, None, slot=NS)
    for s in slots:
        model.set_sampling(do_sample=True, temperature=0.8, top_p=0.95, seed=100 + s, bad_ids=[cfg.image_token_id], slot=s)
        model.kv_fork(NS, s, ids.numel())
    half = args.window // 2
    times = {d: [] for d in DEPTHS}
    model.decode_batch_launch(slots)
    model.synchronize()
    last = max(DEPTHS) + half
    t_prev = time.perf_counter()
    for step in range(1, last + 1):          # step k: the slots hold k private rows when it is launched
        model.decode_batch_launch(slots)
        model.decode_batch_wait()
        t = time.perf_counter()
        for d in DEPTHS:
            if d - half <= step < d + half:
                times[d].append((t - t_prev) * 1e3)
        t_prev = t
    model.decode_batch_wait()
    res = {"model": args.model, "weight_format": args.weight_format, "kv_format": args.kv_format, "slots": NS, "prefix": int(ids.numel()),
           "window": args.window, "fp8_mfma": int(model.stats().get("last_batch_step_fp8_mfma", 0)),
           "step_ms": {str(d): {"median": statistics.median(v), "min": min(v), "max": max(v)} for d, v in times.items()}}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
