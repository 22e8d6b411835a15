"""TikZero adapter timings at the detikzify-v2.5-8b shapes (seeded weights; Llama-3.2-1B embedding model, every_n = 1): the
embedding pass at 64 and 512 tokens, the text-conditioned ViT pass against the plain one, and a text prompt's time to first token
(prefill with a new text, and with the text's cross-attention keys already cached).  One JSON line; --out also writes it to a file.
Every call is synchronous (the C ABI returns after its stream has drained), so host wall time = device time + launch overhead."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def _ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="detikzify-v2.5-8b")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from detikzify_amd.model import load
    from detikzify_amd.util.synthetic import sketch_image
    model, proc = load(a.model, synthetic=1234, adapter=True)
    enc = proc(images=sketch_image(0, 420), return_tensors="pt")
    ids, px = enc.input_ids[0], enc.pixel_values
    V = model.adapter_config.vocab
    texts = iter(torch.randint(0, V, (4096, 64), generator=torch.Generator().manual_seed(0)))
    r = {"model": a.model, "every_n": model.adapter_config.every_n}
    for T in (64, 512):
        t = torch.randint(0, V, (T,), generator=torch.Generator().manual_seed(T))
        r[f"embed_pass_ms_T{T}"] = _ms(lambda: model.embed_text(t), a.reps)
    t64 = torch.randint(0, V, (64,), generator=torch.Generator().manual_seed(64))
    r["vit_plain_ms"] = _ms(lambda: model.vit_encode(px, want_pooled=False), a.reps)
    r["vit_text_cached_ms"] = _ms(lambda: model.vit_encode(px, want_pooled=False, adapter_input_ids=t64), a.reps)
    r["vit_text_new_text_ms"] = _ms(lambda: model.vit_encode(px, want_pooled=False, adapter_input_ids=next(texts)), a.reps)
    r["ttft_image_only_ms"] = _ms(lambda: model.prefill(ids, px, reuse=False), a.reps)
    r["ttft_text_new_text_ms"] = _ms(lambda: model.prefill(ids, px, reuse=False, adapter_input_ids=next(texts)), a.reps)
    r["ttft_text_only_new_text_ms"] = _ms(lambda: model.prefill(ids, None, reuse=False, adapter_input_ids=next(texts)), a.reps)
    r["text_tokens"] = 64
    line = json.dumps(r)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
