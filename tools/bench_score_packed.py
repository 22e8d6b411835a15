#!/usr/bin/env python
"""N candidate programs of one image: N x model.score(prompt + candidate, reuse=True) — the image prefix kept between the calls, the
decoder's weights streamed once per call — against ONE model.score_candidates call (dtk_score_packed: one stream for all rows).
Synthetic weights, one image, (N, tokens per candidate) = (4, 200), (16, 200), (64, 50); max_positions sized to fit them.  Warm
(the prompt cached, workspaces allocated), median of --reps, two clocks: the library's HIP events on the call's stream
(stats.last_prefill_ms, summed over the calls of a side) and host wall time around the Python calls.
Writes profiles/score_packed_<model>.json.
    python tools/bench_score_packed.py [--model detikzify-ds-7b]"""
import argparse, json, statistics, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
from detikzify_amd.model import load, preset
from detikzify_amd.util.image import expand
from detikzify_amd.util.synthetic import sketch_image

CASES = ((4, 200), (16, 200), (64, 50))

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="detikzify-ds-7b")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()

img = sketch_image(0, 224); img = expand(img, max(img.size), do_trim=True)
need = preset(args.model).num_patches + 16 + max(n * t for n, t in CASES)      # the image placeholders + the processor's few text tokens
model, proc = load(args.model, synthetic=1234, max_positions=(need + 63) // 64 * 64)
enc = proc(images=img, return_tensors="pt")
prefix, px = enc.input_ids[0], enc.pixel_values
P = int(prefix.numel())
g = torch.Generator().manual_seed(5)


def sequential(cands):
    ms, t0 = 0.0, time.perf_counter()
    for c in cands:
        model.score(torch.cat([prefix, c]), px, first=P, reuse=True)
        ms += model.stats()["last_prefill_ms"]
    return ms, (time.perf_counter() - t0) * 1e3


def packed(cands):
    t0 = time.perf_counter()
    model.score_candidates(prefix, cands, px, reuse=True)
    return model.stats()["last_prefill_ms"], (time.perf_counter() - t0) * 1e3


rows = []
for n, t in CASES:
    cands = [torch.randint(10, 1000, (t,), generator=g) for _ in range(n)]
    seq, pk = [], []
    for r in range(args.warmup + args.reps):          # the two sides alternate: drift falls on both alike
        seq.append(sequential(cands))
        pk.append(packed(cands))
    seq, pk = seq[args.warmup:], pk[args.warmup:]
    med = lambda xs, k: statistics.median(x[k] for x in xs)
    row = dict(candidates=n, tokens_each=t, rows_packed=n * t,
               sequential_event_ms=round(med(seq, 0), 3), packed_event_ms=round(med(pk, 0), 3),
               sequential_wall_ms=round(med(seq, 1), 3), packed_wall_ms=round(med(pk, 1), 3))
    row["event_ratio"] = round(row["sequential_event_ms"] / row["packed_event_ms"], 2)
    row["wall_ratio"] = round(row["sequential_wall_ms"] / row["packed_wall_ms"], 2)
    rows.append(row)
    print(json.dumps(row), flush=True)
res = dict(model=args.model, prompt_tokens=P, max_positions=int(model.config.max_positions), reps=args.reps, warmup=args.warmup, cases=rows)
out = Path(args.out) if args.out else Path(__file__).resolve().parents[1] / "profiles" / f"score_packed_{args.model.replace('detikzify-', '')}.json"
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text(json.dumps(res, indent=1) + "\n")
print(f"wrote {out}")
