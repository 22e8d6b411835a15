"""
DetikzifyPipeline — the sample() / simulate() front-end over DetikzifyGenerator (behaviour of reference
detikzify/infer/generate.py:356-467: sampling defaults temperature 0.8 / top-p 0.95, `metric` "model" = SelfSim,
"fast" = compiler diagnostics, image loading + trimming).
"""
from __future__ import annotations

from typing import Any, Dict, Generator, List, Literal, Optional, Tuple, Union

from PIL import Image

from ..evaluate.imagesim import ImageSim
from ..util import expand, load
from ..util import unwrap_processor as unwrap
from .generate import DetikzifyGenerator
from .tikz import TikzDocument
from .tree import Numeric


class DetikzifyPipeline:
    def __init__(self, model, processor, temperature: float = 0.8, top_p: float = 0.95, top_k: int = 0,
                 compile_timeout: Optional[int] = 60,
                 metric: Union[Literal["model", "fast"], Any] = "model", **gen_kwargs):
        self.model, self.processor = model, processor
        if metric == "model":      # SelfSim
            # the features of the input image are the same for every rollout: memoised by image bytes (the
            # reference recomputes them per reward, detikzify/evaluate/imagesim.py:91-125 — same value, one ViT pass less)
            self.metric = ImageSim.from_detikzify(model, processor, sync_on_compute=False, cache_reference=True)
        elif metric == "fast":     # compiler diagnostics
            self.metric = None
        else:
            self.metric = metric
        self.gen_kwargs: Dict[str, Any] = {**dict(
            temperature=temperature, top_p=top_p, top_k=top_k,
            max_length=unwrap(processor).tokenizer.model_max_length,
            do_sample=True, compile_timeout=compile_timeout), **gen_kwargs}

    def load(self, image: Union[Image.Image, str], preprocess: bool = True) -> Image.Image:
        image = load(image)
        return expand(image, max(image.size), do_trim=True) if preprocess else image

    def check_inputs(self, image, text):
        # (the adapter's processor nests the model's: a text only reaches the tower through it, reference adapter/__init__.py)
        assert text is None or (hasattr(self.model, "adapter") and unwrap(self.processor) is not self.processor), \
            "You need to load an adapter for textual inputs!"
        assert image or text, "Either image or text (or both) required!"

    def _generator(self, image, text, preprocess, **kw) -> DetikzifyGenerator:
        self.check_inputs(image, text)
        if kw.get("negative_image") is not None:        # guidance_scale's negative image goes the way of the image itself
            kw = {**kw, "negative_image": self.load(kw["negative_image"], preprocess=preprocess)}
        return DetikzifyGenerator(
            model=self.model, processor=self.processor,
            image=self.load(image, preprocess=preprocess) if image is not None else None,
            text=text, **{**self.gen_kwargs, **kw})

    def sample(self, image=None, text: Optional[str] = None, preprocess: bool = True, return_logprobs: bool = False,
               top_logprobs: Optional[int] = None, **gen_kwargs) -> TikzDocument:
        """One sampled TikZ program for the image.  return_logprobs=True attaches `.token_logprobs` and `.token_sample_logprobs` to
        the document: per generated token (EOS included) the model's log-probability of it — comparable with score() — and the log
        of the probability the sampler (temperature, top-k, top-p, min_p, epsilon_cutoff, presence_penalty, frequency_penalty,
        dry_multiplier / dry_base / dry_allowed_length / dry_sequence_breakers, min_new_tokens, exponential_decay_length_penalty,
        logit_bias / sequence_bias: all gen_kwargs, here and in simulate) chose it with.  top_logprobs=k (1 .. 8, with return_logprobs=True)
        also attaches `.token_top_ids` / `.token_top_logprobs`: per generated token the k most likely tokens at its position.

        guidance_scale=g (with negative_image= / negative_text=; gen_kwargs too, here and in simulate, sequential or trees=N): classifier-free
        guidance of model.generate against a negative prompt — by default a white canvas of the processor's size; a text-only prompt
        needs negative_text.  The model must have been loaded with batch_slots >= 2.  Under guidance the attached log-probabilities
        and alternatives describe the guided distribution."""
        from ..model.modeling import check_top_logprobs
        check_top_logprobs(top_logprobs, return_logprobs)
        return self._generator(image, text, preprocess, **gen_kwargs).sample(return_logprobs=return_logprobs, top_logprobs=top_logprobs)

    def score(self, image=None, code: str = "", text: Optional[str] = None, preprocess: bool = True, top_logprobs: Optional[int] = None):
        """(log-probability of `code`, its per-token log-probabilities) under the model, after the prompt sample() builds for
        (image, text).  `code` is tokenised as the generator's output would be — no special tokens, EOS appended — and scored in one
        teacher-forced pass (model.score).  top_logprobs=k: a third and fourth element, per token the k most likely token ids at its
        position and their log-probabilities."""
        import torch
        from ..model.modeling import check_top_logprobs
        check_top_logprobs(top_logprobs)
        self.check_inputs(image, text)
        tokenizer = unwrap(self.processor).tokenizer
        features = self.processor(images=self.load(image, preprocess=preprocess) if image is not None else None, text=text,
                                  text_kwargs={"truncation": True}, return_tensors="pt")
        prompt = features.input_ids.reshape(-1).to(torch.int64)
        program = list(tokenizer.encode(code, add_special_tokens=False)) + [int(tokenizer.eos_token_id)]
        ids = torch.cat([prompt, torch.tensor(program, dtype=torch.int64)])
        conditioning = {name: value for name, value in features.items() if name.startswith("adapter")}     # as DetikzifyGenerator.generate
        top = {"top_logprobs": top_logprobs} if top_logprobs else {}
        out = self.model.score(ids, features.get("pixel_values"), first=prompt.numel(), **conditioning, **top)
        per_token = [float(v) for v in out.logprobs]
        if top:
            return float(out.logprobs.sum(dtype=torch.float64)), per_token, out.top_ids.tolist(), out.top_logprobs.tolist()
        return float(out.logprobs.sum(dtype=torch.float64)), per_token

    def score_candidates(self, image=None, codes: List[str] = (), text: Optional[str] = None,
                         preprocess: bool = True, top_logprobs: Optional[int] = None) -> List[Tuple]:
        """score() of every program in `codes` for one (image, text) — same prompt, same tokenisation (no special tokens, EOS
        appended) — from one packed pass over all of them (model.score_candidates); one (sum, per-token) pair per code, in order
        (with top_logprobs=k: the four elements score() returns)."""
        import torch
        from ..model.modeling import check_top_logprobs
        check_top_logprobs(top_logprobs)
        self.check_inputs(image, text)
        tokenizer = unwrap(self.processor).tokenizer
        features = self.processor(images=self.load(image, preprocess=preprocess) if image is not None else None, text=text,
                                  text_kwargs={"truncation": True}, return_tensors="pt")
        prompt = features.input_ids.reshape(-1).to(torch.int64)
        programs = [torch.tensor(list(tokenizer.encode(code, add_special_tokens=False)) + [int(tokenizer.eos_token_id)], dtype=torch.int64)
                    for code in codes]
        conditioning = {name: value for name, value in features.items() if name.startswith("adapter")}     # as DetikzifyGenerator.generate
        top = {"top_logprobs": top_logprobs} if top_logprobs else {}
        outs = self.model.score_candidates(prompt, programs, features.get("pixel_values"), **conditioning, **top)
        if top:
            return [(float(o.logprobs.sum(dtype=torch.float64)), [float(v) for v in o.logprobs], o.top_ids.tolist(), o.top_logprobs.tolist())
                    for o in outs]
        return [(float(o.logprobs.sum(dtype=torch.float64)), [float(v) for v in o.logprobs]) for o in outs]

    def simulate(self, image=None, text: Optional[str] = None, preprocess: bool = True,
                 expansions: Optional[Numeric] = None, timeout: Optional[int] = None, trees: int = 1,
                 **gen_kwargs) -> Generator[Tuple[Numeric, TikzDocument], None, None]:
        """MCTS: yields (score, document) for every rollout until `expansions` / `timeout`.

        `trees` > 1 (not in the reference): that many independent searches of the same image (and / or text) decoded as ONE
        batch on this GPU (infer/batching.py; the model must have been loaded with batch_slots > trees), each with its own
        `expansions` / `timeout` budget — root parallelisation; results arrive in completion order.  guidance_scale= (with
        negative_image= / negative_text=) works here too: every tree then decodes in two of the engine's slots (its own and the
        negative branch's), so at most decode_slots // 2 trees decode at once and the rest take turns.

        top_logprobs=j (1 .. 8, sequential or trees=N): every yielded document carries `.token_logprobs` / `.token_sample_logprobs` /
        `.token_top_ids` / `.token_top_logprobs`, one entry per token behind the prompt, as sample(return_logprobs=True,
        top_logprobs=j) attaches them; with trees > 1 the batch engine is built with top_logprobs=j."""
        if trees > 1:
            from .batching import simulate_parallel
            assert preprocess, "parallel trees take the default preprocessing"
            self.check_inputs(image, text)
            yield from simulate_parallel(self, image, trees=trees, expansions_per_tree=expansions or None,
                                         mcts_timeout=timeout or None, text=text, **gen_kwargs)
            return
        generator = self._generator(image, text, preprocess, metric=self.metric,
                                    mcts_timeout=timeout or None, **gen_kwargs)
        yield from generator.simulate(expansions or None)

    def __call__(self, *args, **kwargs) -> TikzDocument:
        return self.sample(*args, **kwargs)
