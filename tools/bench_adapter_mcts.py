"""Text-conditioned (TikZero) MCTS throughput at the detikzify-v2.5-8b shapes: seeded weights and adapter (Llama-3.2-1B embedding
model), a text-only prompt (the adapter's dummy image), the stub SelfSim reward of bench.py --full's MCTS phase (device ViT on
SyntheticTikzDocument renderings, reference features cached).  Rollouts/s of one tree (the sequential search), of 64 trees of one
text, of 8 texts x 8 trees, and — in the same process — of 64 image-only trees, each with the engine's wait_s / seconds.
One JSON line; --out also writes it to a file."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

TEXTS = ["a red circle inside a blue square", "a directed graph with four nodes", "a bar chart of three values",
         "two overlapping ellipses", "a right triangle with labelled sides", "a sine wave on labelled axes",
         "a binary tree of depth three", "a flow chart with a decision diamond"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="detikzify-v2.5-8b")
    ap.add_argument("--new-tokens", type=int, default=96)
    ap.add_argument("--seq-expansions", type=int, default=3)
    ap.add_argument("--expansions", type=int, default=2, help="expansions per tree of the batched searches")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from detikzify_amd.infer import DetikzifyPipeline, SyntheticTikzDocument
    from detikzify_amd.infer.batching import simulate_parallel_images
    from detikzify_amd.model import load
    from detikzify_amd.util.synthetic import sketch_image
    t0 = time.perf_counter()
    model, proc = load(a.model, synthetic=1234, adapter=True, batch_slots=72, max_positions=512)
    load_s = time.perf_counter() - t0
    T0 = int(proc(text=TEXTS[0], return_tensors="pt")["input_ids"].shape[1])
    pipe = DetikzifyPipeline(model, proc, metric="model", document_class=SyntheticTikzDocument, max_length=T0 + a.new_tokens,
                             compile_timeout=None)
    pipe.metric.cache_reference = True
    img = sketch_image(0, 224)

    def run(images, texts, trees_per_image, expansions):
        s0 = model.stats()
        t = time.perf_counter()
        n = sum(1 for _ in simulate_parallel_images(pipe, images, trees_per_image, expansions, texts=texts,
                                                     seeds=[1000 + k for k in range(len(images) * trees_per_image)]))
        sec = time.perf_counter() - t
        out = {"trees": len(images) * trees_per_image, "expansions_per_tree": expansions, "rollouts": n, "seconds": round(sec, 3),
               "rollouts_per_sec": round(n / sec, 3), "vit_passes": model.stats()["vit_images"] - s0["vit_images"]}
        eng = getattr(model, "last_batch_stats", None) if len(images) * trees_per_image > 1 else None
        if eng:
            out.update(wait_s_over_seconds=round(eng["wait_s"] / sec, 3), join_s=eng["prefill_s"], idle_s=eng["idle_between_steps_s"],
                       prefix_encodes=eng["prefix_encodes"], resumed_in_place=eng["resumed_in_place"], steps=eng["steps"],
                       tokens_out=eng["tokens_out"])
        model.last_batch_stats = None
        return out

    r = {"model": a.model, "load_s": round(load_s, 1), "prompt_tokens": T0, "new_tokens": a.new_tokens,
         "reward": "stub SelfSim (device ViT of SyntheticTikzDocument renderings, reference features cached); not LaTeX"}
    run([img], None, 4, 1)                                                            # warm-up (graphs, kernels)
    r["image_only_64_trees"] = run([img], None, 64, a.expansions)
    r["text_1_tree_sequential"] = run([None], [TEXTS[0]], 1, a.seq_expansions)
    r["text_64_trees_one_text"] = run([None], [TEXTS[0]], 64, a.expansions)
    r["text_8_texts_x_8_trees"] = run([None] * 8, TEXTS, 8, a.expansions)
    r["text64_over_image64"] = round(r["text_64_trees_one_text"]["rollouts_per_sec"] / r["image_only_64_trees"]["rollouts_per_sec"], 3)
    r["text64_over_sequential"] = round(r["text_64_trees_one_text"]["rollouts_per_sec"] / r["text_1_tree_sequential"]["rollouts_per_sec"], 2)
    line = json.dumps(r)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
