#!/usr/bin/env python
"""What prompt-lookup speculative decoding costs and buys: in ONE process, alternating, on a model loaded with
batch_slots=4 (the multi-vector family) and the same model loaded with batch_slots=0,
  * "slot":    plain steps of slot 0 (the 1-vector step the speculative run is bit-identical to): step time, tokens/s;
  * "single":  the single-sequence step of the batch_slots=0 context (13-bit planes, split-K attention): step time, tokens/s;
  * "spec_k1_a<A>" / "spec_k3_a<A>": speculative steps with K = 1 (2-vector step) / K = 3 (4-vector step) whose drafts come from a
    host table that makes every step accept exactly A drafts (A + 1 tokens): step time, tokens/s;
and the two speculative kernels' own time per step from HIP events around back-to-back launches (dtk_bench_spec).  From these: the
break-even tokens per step against both baselines (spec step time / baseline step time) — the acceptance below which the feature loses.
Synthetic weights, real shapes: the acceptance a real checkpoint reaches on real TikZ is NOT measured here.
Writes profiles/spec_<model>.json."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def corpus_cost(args):
    """--corpus-ids: the COST of a corpus, nothing else.  The lookup source at K = 3 over a sampled run of slot 0, with a corpus of n
    copies of an id the sequence never holds (the image placeholder: banned from sampling, absent from the prompt), so no window
    matches and every corpus size decodes the same tokens with the same drafts.  Per size, alternating in one process: the step time
    (one step in flight, as generate() keeps it) and the step's own kernels from HIP events around back-to-back launches
    (dtk_bench_spec: k_spec_accept + k_spec_draft, with k_spec_corpus between them when a corpus is set).  What a corpus BUYS — the
    acceptance on real TikZ — is not measured here."""
    from detikzify_amd.model import load
    sizes = [int(v) for v in args.corpus_ids.split(",")]
    model, _ = load(args.model, synthetic=1234, max_positions=2048, batch_slots=4)
    cfg = model.config
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab - 1, (args.prompt + 8,), generator=g)
    ids = ids[ids != cfg.image_token_id][:args.prompt].contiguous()
    T = int(ids.numel())
    samp = dict(do_sample=True, temperature=0.8, top_p=0.95, seed=7, bad_ids=[cfg.image_token_id])
    warm, K = 8, 3
    assert T + 4 * (args.steps + warm + 4) + 8 < 2048, "fewer steps or a shorter prompt: a step accepts up to 4 tokens"
    legs = [f"corpus_{n}" for n in sizes]
    res = {"model": args.model, "vocab": int(cfg.vocab), "prompt_tokens": T, "timed_steps": args.steps, "K": K, "max_ngram": args.ngram,
           "step_us": {k: [] for k in legs}, "kernels_us_per_step": {k: [] for k in legs}, "tokens": {}}

    def leg(n):
        if n:
            model.spec_set_corpus([[int(cfg.image_token_id)] * n])
        model.set_sampling(slot=0, **samp)
        model.prefill(ids, None, slot=0)
        model.spec_begin(K, args.ngram)
        kept = T
        try:
            toks = []
            for _ in range(warm):
                model.spec_launch(); toks += model.spec_wait()
            model.spec_launch()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                model.spec_launch(); toks += model.spec_wait()
            dt = time.perf_counter() - t0
            toks += model.spec_wait()
            kept = T + len(toks)
            us = C.c_float(0)
            model._check(model.lib.dtk_bench_spec(model._ctx, 50, C.byref(us)), "dtk_bench_spec")
        finally:
            model.spec_end(kept)
            if n:
                model.spec_set_corpus([])
        return dt / args.steps, float(us.value), toks

    for _ in range(args.rounds):
        for n in sizes:
            step_s, us, toks = leg(n)
            res["step_us"][f"corpus_{n}"].append(round(step_s * 1e6, 2))
            res["kernels_us_per_step"][f"corpus_{n}"].append(round(us, 3))
            assert res["tokens"].setdefault("first", toks) == toks, "a corpus that cannot match changed the tokens"
    res["tokens"] = {"per_leg": len(res["tokens"]["first"])}
    res["median_step_us"] = {k: round(statistics.median(v), 2) for k, v in res["step_us"].items()}
    res["median_kernels_us_per_step"] = {k: round(statistics.median(v), 3) for k, v in res["kernels_us_per_step"].items()}
    out = Path(args.out) if args.out else ROOT / "profiles" / f"spec_corpus_{args.model.replace('detikzify-', '')}.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="detikzify-ds-7b")
    ap.add_argument("--prompt", type=int, default=300, help="prompt tokens (text only)")
    ap.add_argument("--steps", type=int, default=160, help="timed steps per leg")
    ap.add_argument("--rounds", type=int, default=3, help="alternations")
    ap.add_argument("--out", default=None)
    ap.add_argument("--corpus-ids", default=None, help="comma-separated corpus sizes, e.g. 0,4096,65536: measure what a prompt-lookup "
                                                       "corpus costs instead (writes profiles/spec_corpus_<model>.json)")
    ap.add_argument("--ngram", type=int, default=16, help="--corpus-ids: max_matching_ngram_size of the lookup")
    args = ap.parse_args()
    if args.corpus_ids is not None:
        return corpus_cost(args)
    from detikzify_amd.model import load
    model, _ = load(args.model, synthetic=1234, max_positions=2048, batch_slots=4)
    lone, _ = load(args.model, synthetic=1234, max_positions=2048, batch_slots=0)
    cfg = model.config
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab - 1, (args.prompt + 8,), generator=g)
    ids = ids[ids != cfg.image_token_id][:args.prompt].contiguous()
    T = int(ids.numel())
    samp = dict(do_sample=True, temperature=0.8, top_p=0.95, seed=7, bad_ids=[cfg.image_token_id])
    warm = 8
    n_truth = 4 * (args.steps + warm + 4) + 8
    assert T + n_truth < 2048, "fewer steps or a shorter prompt: the forced runs accept up to 4 tokens per step"
    legs = ["slot", "single"] + [f"spec_k1_a{a}" for a in (0, 1)] + [f"spec_k3_a{a}" for a in (0, 1, 2, 3)]
    res = {"model": args.model, "vocab": int(cfg.vocab), "prompt_tokens": T, "timed_steps": args.steps,
           "step_us": {k: [] for k in legs}, "tok_s": {k: [] for k in legs}, "kernels_us_per_step": None}

    # the plain run of slot 0: the sequence every forced table is cut from
    model.set_sampling(slot=0, **samp)
    model.prefill(ids, None, slot=0)
    truth = []
    for _ in range(n_truth):
        model.decode_batch_launch([0])
        truth.append(model.decode_batch_wait()[0])

    def slot():
        model.set_sampling(slot=0, **samp)
        model.prefill(ids, None, slot=0)
        for _ in range(warm):
            model.decode_batch_launch([0]); model.decode_batch_wait()
        model.decode_batch_launch([0])
        t0 = time.perf_counter()
        for _ in range(args.steps):        # one step always in flight, as generate() keeps it
            model.decode_batch_launch([0]); model.decode_batch_wait()
        dt = time.perf_counter() - t0
        model.decode_batch_wait()
        return dt / args.steps, args.steps / dt

    def single():
        lone.set_sampling(**samp)
        lone.prefill(ids, None)
        for _ in range(warm):
            lone.decode_launch(); lone.decode_wait()
        lone.decode_launch()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            lone.decode_launch(); lone.decode_wait()
        dt = time.perf_counter() - t0
        lone.decode_wait()
        return dt / args.steps, args.steps / dt

    def table(a, K):
        """drafts that make every step behind the first accept exactly a of its K drafts: the step that starts at position p carries
        the right ids at p .. p + a - 1 and a wrong one at p + a"""
        tab = [-1] * T + list(truth)
        p = T + 1
        while a < K and p + a < len(tab):
            wrong = tab[p + a] + 1
            tab[p + a] = wrong if wrong < cfg.vocab - 1 and wrong != cfg.image_token_id else tab[p + a] - 1
            p += a + 1
        return tab

    def spec(K, a):
        model.set_sampling(slot=0, **samp)
        model.prefill(ids, None, slot=0)
        model.spec_begin(K, 2, table=True)
        kept = T
        try:
            model.spec_set_drafts(table(a, K))
            toks = []
            for _ in range(warm):
                model.spec_launch(); toks += model.spec_wait()
            model.spec_launch()
            n0 = len(toks)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                model.spec_launch(); toks += model.spec_wait()
            dt = time.perf_counter() - t0
            toks += model.spec_wait()
            made = len(toks) - n0 - (a + 1)       # (the tokens of the steps read inside the timed loop)
            assert toks == truth[:len(toks)], "the speculative run left the plain run's sequence"
            assert made == args.steps * (a + 1), (made, args.steps, a)
            kept = T + len(toks)
            if res["kernels_us_per_step"] is None and K == 3:
                us = C.c_float(0)
                model._check(model.lib.dtk_bench_spec(model._ctx, 50, C.byref(us)), "dtk_bench_spec")
                res["kernels_us_per_step"] = {"k_spec_accept+k_spec_draft": round(float(us.value), 3)}
        finally:
            model.spec_end(kept)
        return dt / args.steps, made / dt

    run = {"slot": slot, "single": single}
    for K, accs in ((1, (0, 1)), (3, (0, 1, 2, 3))):
        for a in accs:
            run[f"spec_k{K}_a{a}"] = (lambda K=K, a=a: spec(K, a))
    for _ in range(args.rounds):
        for leg in legs:
            step_s, tok_s = run[leg]()
            res["step_us"][leg].append(round(step_s * 1e6, 2))
            res["tok_s"][leg].append(round(tok_s, 2))
    med_us = {k: statistics.median(v) for k, v in res["step_us"].items()}
    res["median_step_us"] = {k: round(v, 2) for k, v in med_us.items()}
    res["median_tok_s"] = {k: round(statistics.median(v), 2) for k, v in res["tok_s"].items()}
    for K, accs in ((1, (0, 1)), (3, (0, 1, 2, 3))):
        step = statistics.median([med_us[f"spec_k{K}_a{a}"] for a in accs])
        res[f"spec_k{K}_step_us"] = round(step, 2)
        # tokens a step must accept on average to match the baseline's rate: below it the feature loses
        res[f"break_even_tokens_per_step_k{K}"] = {"vs_slot": round(step / med_us["slot"], 4), "vs_single": round(step / med_us["single"], 4)}
    out = Path(args.out) if args.out else ROOT / "profiles" / f"spec_{args.model.replace('detikzify-', '')}.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
