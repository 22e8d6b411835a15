#!/usr/bin/env python
"""Teacher-forced scoring against what it replaces, at the image prefix + N program tokens (device times from the library's own HIP
events on the call's stream — stats.last_prefill_ms, ViT included on both sides; medians of --reps after --warmup):
  (a) dtk_prefill of the same ids: everything but the lm_head pass over all rows;
  (b) dtk_score;
  (c) N x the single-sequence decode step measured in the same process: what the same N numbers cost through decode + get_logits.
(a) and (b) alternate; the median of their paired differences is the log-softmax lm_head pass (final norm, GEMM with the folded epilogue, record merge); its TFLOP/s counts 2 N V d.
Writes profiles/score_<model>.json.
    python tools/bench_score.py [--model detikzify-ds-7b] [--tokens 512]"""
import argparse, json, statistics, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
from detikzify_amd.model import load
from detikzify_amd.util.image import expand
from detikzify_amd.util.synthetic import sketch_image

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="detikzify-ds-7b")
ap.add_argument("--weight-format", default="bf16")
ap.add_argument("--tokens", type=int, default=512)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
model, proc = load(args.model, synthetic=1234, weight_format=args.weight_format)
model.reuse_prefix = False
img = sketch_image(0, 224); img = expand(img, max(img.size), do_trim=True)
enc = proc(images=img, return_tensors="pt")
g = torch.Generator().manual_seed(5)
prog = torch.randint(10, 1000, (args.tokens,), generator=g)
ids, px = torch.cat([enc.input_ids[0], prog]), enc.pixel_values
first = enc.input_ids[0].numel()


# (a) and (b) alternate, so clock and temperature drift falls on both alike; the lm_head pass is the median of the PAIRED differences
ms_a, ms_b = [], []
for r in range(args.warmup + args.reps):
    model.prefill(ids, px, reuse=False)
    ms_a.append(model.stats()["last_prefill_ms"])
    model.score(ids, px, first=first, reuse=False)
    ms_b.append(model.stats()["last_prefill_ms"])
ms_a, ms_b = ms_a[args.warmup:], ms_b[args.warmup:]
a, b = statistics.median(ms_a), statistics.median(ms_b)
pass_ms = statistics.median([y - x for x, y in zip(ms_a, ms_b)])
model.set_sampling(do_sample=False)
model.prefill(ids[:first + args.tokens // 2], px, reuse=False)          # decode steps at the middle context length
steps = []
for r in range(args.warmup + args.reps):
    t0 = time.perf_counter()
    for _ in range(8):
        model.decode_launch(); model.decode_wait()
    steps.append((time.perf_counter() - t0) / 8 * 1e3)
step = statistics.median(steps[args.warmup:])
c = args.tokens * step
cfg = model.config
flop = 2.0 * args.tokens * cfg.vocab * cfg.hidden
res = dict(model=args.model, weight_format=args.weight_format, rows=int(ids.numel()), scored_tokens=args.tokens,
           prefill_ms=round(a, 3), score_ms=round(b, 3), decode_step_ms=round(step, 4), decode_steps_total_ms=round(c, 1),
           lm_head_pass_ms=round(pass_ms, 3), lm_head_pass_tflops=round(flop / max(pass_ms, 1e-6) / 1e9, 1),
           prefill_ms_min_max=[round(min(ms_a), 3), round(max(ms_a), 3)], score_ms_min_max=[round(min(ms_b), 3), round(max(ms_b), 3)],
           score_vs_decode_speedup=round(c / b, 1), workspace_bytes=cfg.max_positions * ((cfg.vocab + 127) // 128) * 16,
           reps=args.reps, warmup=args.warmup)
print(json.dumps(res))
out = Path(args.out) if args.out else Path(__file__).resolve().parents[1] / "profiles" / f"score_{args.model.replace('detikzify-', '')}.json"
out.write_text(json.dumps(res, indent=1) + "\n")
