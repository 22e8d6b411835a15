#!/usr/bin/env python
"""Guided rollouts in the batch engine's slots ("standing pairs"): what they cost, in ONE process per leg.

  --leg recapture   the wall time of the first dtk_decode_batch_launch after a dtk_set_guidance against a steady launch, on a step of
                    --slots active slots: what a change of the pair set costs when it drops the captured steps, and — with
                    --reserve P — what it costs with standing pairs.  Uses only entry points the previous release has, so
                    --tree <checkout> measures another build (the parent commit's) with this very script.
  --leg blocks      dtk_bench_cfg (HIP events around back-to-back launches of the guidance kernels) with 1 live pair and a reservation
                    of 0, 1, 8 and 32 pairs: what the empty blocks of a standing table cost.
  --leg rollouts    rollouts through model.generate under the native engine: --guided G guided rollouts (2 G slots) or --plain N
                    unguided ones, an image prefix of the model's patch count + --new new tokens each: rollouts/s, step rate and the
                    share of the wall time the engine spent waiting for the device (wait_s / seconds).
Synthetic weights, real shapes.  Appends its result to profiles/cfg_engine_<model>.json under the leg's name."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import threading
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="detikzify-ds-7b")
    ap.add_argument("--leg", choices=("recapture", "blocks", "rollouts"), required=True)
    ap.add_argument("--tree", default=None, help="another checkout whose build is measured (leg recapture)")
    ap.add_argument("--slots", type=int, default=64, help="active slots of the step (recapture) / decode slots of the engine (rollouts)")
    ap.add_argument("--reserve", type=int, default=0, help="standing pairs (recapture)")
    ap.add_argument("--guided", type=int, default=0)
    ap.add_argument("--plain", type=int, default=0)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--prompt", type=int, default=64, help="prompt tokens of the recapture / blocks legs (text only)")
    ap.add_argument("--scale", type=float, default=2.0)
    ap.add_argument("--name", default=None, help="key of the result in the output file")
    ap.add_argument("--out", default=None)
    ap.add_argument("--load", default="", help="extra load() arguments as k=v,k=v (e.g. weight_format=fp8)")
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.tree).resolve() if args.tree else ROOT))
    from detikzify_amd.model import load
    extra = {k: (int(v) if v.isdigit() else v) for k, v in (kv.split("=") for kv in args.load.split(",") if kv)}
    res = {"model": args.model, "leg": args.leg, "tree": args.tree or "."}

    if args.leg in ("recapture", "blocks"):
        n = args.slots if args.leg == "recapture" else 2
        model, _ = load(args.model, synthetic=1234, max_positions=2048, batch_slots=n + 1 if n > 4 else 5, **extra)
        cfg = model.config
        g = torch.Generator().manual_seed(1)
        ids = torch.randint(3, cfg.vocab - 1, (args.prompt + 8,), generator=g)
        ids = ids[ids != cfg.image_token_id][:args.prompt].contiguous()
        samp = dict(do_sample=True, temperature=0.8, top_p=0.95, bad_ids=[cfg.image_token_id])
        active = list(range(n))
        for s in active:
            model.set_sampling(slot=s, seed=s, **(samp if s % 2 == 0 else {}))
            model.prefill(torch.roll(ids, s), None, slot=s)

        def step_ms():
            model.synchronize()
            t0 = time.perf_counter()
            model.decode_batch_launch(active)
            t1 = time.perf_counter()
            model.decode_batch_wait()
            return (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3

    if args.leg == "recapture":
        if args.reserve:
            model.reserve_guidance(args.reserve)
        model.set_guidance(args.scale, 0, 1)
        for _ in range(6):
            step_ms()
        steady = [step_ms() for _ in range(20)]
        first = []
        for k in range(8):       # a pair joins, a pair leaves, a new scale: every change of the pair set
            if k % 2 == 0:
                model.set_guidance(args.scale, 2, 3)
            else:
                model.set_guidance(None, 2, None)
            first.append(step_ms())
        res.update(active_slots=n, reserved_pairs=args.reserve,
                   steady_launch_ms=round(statistics.median(a for a, _ in steady), 4), steady_step_ms=round(statistics.median(b for _, b in steady), 4),
                   first_launch_after_set_guidance_ms=[round(a, 4) for a, _ in first],
                   first_step_after_set_guidance_ms=[round(b, 4) for _, b in first],
                   median_first_launch_ms=round(statistics.median(a for a, _ in first), 4))
        if hasattr(model, "batch_graph_captures"):
            res["batch_graph_captures"] = model.batch_graph_captures
    elif args.leg == "blocks":
        res["kernels_us"] = {}
        for r in (0, 1, 8, 32):
            model.reserve_guidance(r)
            model.set_guidance(args.scale, 0, 1)
            model.decode_batch_launch([0, 1]); model.decode_batch_wait()
            us = (C.c_float * 2)()
            runs = []
            for _ in range(5):
                model._check(model.lib.dtk_bench_cfg(model._ctx, 50, us), "dtk_bench_cfg")
                runs.append((float(us[0]), float(us[1])))
            res["kernels_us"][f"reserved_{r}"] = {"k_cfg_lse+k_cfg_mix": round(statistics.median(a for a, _ in runs), 3),
                                                   "k_cfg_follow": round(statistics.median(b for _, b in runs), 3)}
            model.set_guidance(None, 0, None)
            for s in (0, 1):
                model.prefill(torch.roll(ids, s), None, slot=s)
        model.reserve_guidance(0)
    else:
        from detikzify_amd.infer.engine import NativeBatchEngine
        n_seq = args.guided or args.plain
        model, proc = load(args.model, synthetic=1234, max_positions=2048, batch_slots=args.slots + 2, **extra)
        cfg = model.config
        n_img = int(cfg.num_patches)
        g = torch.Generator().manual_seed(1)
        ids = torch.full((n_img,), cfg.image_token_id, dtype=torch.int64)
        size = int(cfg.vit_image)
        px = torch.rand((1, 3, size, size), generator=g)
        white = torch.ones_like(px)
        eng = NativeBatchEngine(model, max_batch=2 * args.guided if args.guided else args.plain, guided_pairs=args.guided, gather=n_seq,
                                gather_timeout=60.0)
        kw = dict(input_ids=ids[None], pixel_values=px, do_sample=True, temperature=0.8, top_p=0.95, max_new_tokens=args.new, eos_token_id=-1,
                  bad_words_ids=[[cfg.image_token_id]])
        if args.guided:
            kw.update(guidance_scale=args.scale, negative_pixel_values=white)
        errs = []

        def worker(k):
            try:
                model.generate(seed=100 + k, sequence_owner=k, **kw)
            except BaseException as e:  # noqa: BLE001
                errs.append(e)
        for rnd in range(2):       # the first round warms the captures and the prefix cache
            eng.expect(n_seq, 60.0)
            st0 = eng.native_stats()
            ths = [threading.Thread(target=worker, args=(k,)) for k in range(n_seq)]
            t0 = time.perf_counter()
            [t.start() for t in ths]
            [t.join() for t in ths]
            dt = time.perf_counter() - t0
            if errs:
                raise errs[0]
            st = eng.native_stats()
        res.update(guided=args.guided, plain=args.plain, new_tokens=args.new, prefix_tokens=n_img, seconds=round(dt, 4),
                   rollouts_per_s=round(n_seq / dt, 3), steps=int(st["steps"] - st0["steps"]),
                   steps_per_s=round((st["steps"] - st0["steps"]) / dt, 2), wait_s=round(st["wait_s"] - st0["wait_s"], 4),
                   wait_share=round((st["wait_s"] - st0["wait_s"]) / dt, 4), batch_graph_captures=model.batch_graph_captures)
        eng.close()
    out = Path(args.out) if args.out else ROOT / "profiles" / f"cfg_engine_{args.model.replace('detikzify-', '')}.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    doc = json.loads(out.read_text()) if out.exists() else {}
    doc[args.name or args.leg] = res
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
