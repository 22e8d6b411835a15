"""AdapterProcessor (reference detikzify/model/adapter/processing_adapter.py): the TikZero adapter's processor.  The text goes
to the embedding model's tokenizer as adapter_input_ids / adapter_attention_mask; a prompt without an image gets the processor's
prompt for DUMMY_IMAGE (the tower then sees the adapter's dummy input, not these pixels: they are not returned)."""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import torch
from PIL import Image

from .processing import BatchFeature

# reference detikzify/util/image.py:11
DUMMY_IMAGE = Image.new("RGB", (24, 24), color="white")


class AdapterProcessor:
    def __init__(self, processor, tokenizer):
        if processor is None:
            raise ValueError("You need to specify a `processor`.")
        if tokenizer is None:
            raise ValueError("You need to specify a `tokenizer`.")
        self.processor, self.tokenizer = processor, tokenizer

    def __call__(self, text=None, images=None, return_tensors: Optional[str] = None, text_kwargs: Optional[Dict[str, Any]] = None,
                 images_kwargs: Optional[Dict[str, Any]] = None, **kwargs) -> BatchFeature:
        if images is None and text is None:
            raise ValueError("Either `images` or `text` (or both) are expected as arguments to an `AdapterProcessor` instance.")
        text_kwargs, images_kwargs = dict(text_kwargs or {}), dict(images_kwargs or {})
        text_inputs: Dict[str, Any] = {}
        if text is not None:
            text = [text] if isinstance(text, str) else list(text)
            enc = self.tokenizer(text=text, **kwargs, **text_kwargs)
            text_inputs = {f"adapter_{k}": v for k, v in dict(enc).items()}
            if getattr(self.processor, "model_expects_text", False):
                images_kwargs.update(text=text, add_bos_token=True)
        if images is None:
            image_inputs = self.processor(images=len(text) * [DUMMY_IMAGE], return_tensors=return_tensors, **kwargs, **images_kwargs)
            image_inputs = {k: image_inputs[k] for k in ("input_ids", "attention_mask") if k in image_inputs}
        else:
            n = len(images) if isinstance(images, (list, tuple)) else 1
            if text is not None and n != len(text):
                raise ValueError(f"Received {n} images for {len(text)} prompts. Each prompt should be associated with an image.")
            image_inputs = dict(self.processor(images=images, return_tensors=return_tensors, **kwargs, **images_kwargs).items())
        if return_tensors == "pt" and text_inputs:
            text_inputs = {k: _pad_pt(v, 0 if k.endswith("attention_mask") else getattr(self.tokenizer, "pad_token_id", 0) or 0)
                           for k, v in text_inputs.items()}
        return BatchFeature({**image_inputs, **text_inputs})

    def batch_decode(self, *args, **kwargs):
        return self.processor.batch_decode(*args, **kwargs)

    def decode(self, *args, **kwargs):
        return self.processor.decode(*args, **kwargs)

    @property
    def model_input_names(self) -> List[str]:
        names = list(getattr(self.tokenizer, "model_input_names", ["input_ids", "attention_mask"]))
        return list(dict.fromkeys(names + list(getattr(self.processor, "model_input_names", []))))


def _pad_pt(v, pad: int) -> torch.Tensor:
    """lists of rows -> one int64 tensor (a tokenizer that already returned tensors is left alone); rows of unequal length are
    right-padded (pad id, mask 0) — what a batched HF tokenizer call with padding=True gives"""
    if isinstance(v, torch.Tensor):
        return v
    rows = [list(r) for r in v]
    width = max(len(r) for r in rows)
    return torch.tensor([r + [pad] * (width - len(r)) for r in rows], dtype=torch.int64)
