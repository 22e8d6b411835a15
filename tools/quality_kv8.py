#!/usr/bin/env python
"""What kv_format "mxfp8" does to the logits at full size, on the contexts `act_fp8` was characterised on
(tests/test_gpu_parity_batched.py::test_mxfp8_activations_against_bf16_activations): detikzify-cl-7b, fp8 weights, full depth, the
seed-0 sketch's image prefix forked into 32 slots that sample 16 tokens each (T = .8, top-p .95, seeds 300 + slot) in a bf16-KV
context — 512 contexts.  The same contexts are then teacher-forced (dtk_resume_slot forces the next token) through a SECOND context
of the same model with kv_format="mxfp8", its shadow rows written by its own steps.  Per context: rel-L2 of the MXFP8-KV step's logits
against the bf16-KV step's, and whether the greedy token is the same.  --steps beyond 16 continues the same sequences to greater depth
(the first 16 are reported on their own).  --oracle N: for the first N slots the CPU oracles' own distance at full size — the kv8
oracle (tests/kv8_oracle.py) against the plain bf16-policy oracle on the same 16 contexts.  One process, the two contexts one after
the other.  Writes profiles/kv8_quality_<model>_<weight format>.json."""
from __future__ import annotations

import argparse
import gc
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

CONTEXTS = 32


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="detikzify-cl-7b")
    ap.add_argument("--weight-format", default="fp8")
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--oracle", type=int, default=0, help="slots whose 16 contexts also go through the CPU oracles")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from detikzify_amd.model import load
    from detikzify_amd.util.synthetic import sketch_image
    A, SRC = list(range(CONTEXTS)), CONTEXTS
    res = {"model": args.model, "weight_format": args.weight_format, "contexts": CONTEXTS, "steps": args.steps}

    def context(kv_format):
        model, proc = load(args.model, synthetic=1234, max_positions=512, weight_format=args.weight_format, batch_slots=CONTEXTS + 1, kv_format=kv_format)
        enc = proc(images=sketch_image(0, 224), return_tensors="pt")
        ids, px = enc.input_ids[0], enc.pixel_values
        model.set_sampling(do_sample=False, slot=SRC)
        model.prefill(ids, px, slot=SRC)
        return model, proc, ids, px

    # the contexts: sampled with bf16 key/value rows
    model, proc, ids, px = context("bf16")
    img_tok, n_img = model.config.image_token_id, ids.numel()
    for s in A:
        model.set_sampling(do_sample=True, temperature=0.8, top_p=0.95, top_k=0, seed=300 + s, bad_ids=[img_tok], slot=s)
        model.kv_fork(SRC, s, n_img)
    toks, LA = {s: [] for s in A}, {s: [] for s in A}
    for _ in range(args.steps):
        model.decode_batch_launch(A)
        out = model.decode_batch_wait()
        for s in A:
            toks[s].append(int(out[s]))
            LA[s].append(model.get_logits_slot(s))
    if args.oracle:
        from tests.fullsize import host_side
        from tests.kv8_oracle import Kv8LlamaOracle
        t0 = time.perf_counter()
        hs = host_side(model, proc, args.model, args.weight_format)
        dist, dev = [], []
        for s in A[:args.oracle]:
            _, _, plain, _ = hs.oracles(model, fp32=False)
            _, _, quant, _ = hs.oracles(model, fp32=False)
            llm = Kv8LlamaOracle(quant.llm.cfg, quant.llm.w, quant.llm.precision)
            llm.k, llm.v, llm.pos, llm.kv_from = quant.llm.k, quant.llm.v, quant.llm.pos, n_img
            quant.llm = llm
            rp, rq = plain.extend(toks[s][:16]), quant.extend(toks[s][:16])
            for k in range(16):
                dist.append(rel_l2(rq[k], rp[k]))
                dev.append(rel_l2(LA[s][k], rp[k]))
        res["oracle"] = {"slots": args.oracle, "contexts": len(dist), "kv8_oracle_vs_plain_bf16_oracle": {"mean": statistics.mean(dist), "worst": max(dist)},
                         "bf16_kv_device_vs_plain_bf16_oracle": {"mean": statistics.mean(dev), "worst": max(dev)},
                         "seconds": time.perf_counter() - t0}
        del hs
    del model
    gc.collect()

    # the same contexts, teacher-forced through a kv8 context
    model, proc, ids, px = context("mxfp8")
    key = model.image_key(px)
    for s in A:
        model.set_sampling(do_sample=False, bad_ids=[img_tok], slot=s)
        model.kv_fork(SRC, s, n_img)
    LB = {s: [] for s in A}
    for k in range(args.steps):
        for s in A:
            model.resume_slot(s, torch.cat([ids, torch.tensor(toks[s][:k + 1], dtype=torch.long)]), key)
        model.decode_batch_launch(A)
        out = model.decode_batch_wait()
        for s in A:
            assert int(out[s]) == toks[s][k], (s, k)
            LB[s].append(model.get_logits_slot(s))
    assert all(model.kv8_from(s) == n_img for s in A)

    def figures(lo, hi):
        d = [rel_l2(LB[s][k], LA[s][k]) for s in A for k in range(lo, hi)]
        same = sum(int(LB[s][k].argmax()) == int(LA[s][k].argmax()) for s in A for k in range(lo, hi))
        return {"private_keys": [lo + 1, hi], "contexts": len(d), "rel_l2_mean": statistics.mean(d), "rel_l2_worst": max(d), "same_greedy_token": same}
    res["mxfp8_kv_vs_bf16_kv"] = [figures(0, min(16, args.steps))]
    for lo in range(16, args.steps, 48):
        res["mxfp8_kv_vs_bf16_kv"].append(figures(lo, min(lo + 48, args.steps)))
    line = json.dumps(res, indent=1)
    print(line)
    out = args.out or str(ROOT / "profiles" / f"kv8_quality_{args.model.replace('detikzify-', '')}_{args.weight_format}.json")
    Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
