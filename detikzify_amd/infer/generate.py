"""
DetikzifyGenerator — one image, one search tree (rows a·G, a·R, a·M).  `TikzGenerator` is the alias the north-star names.

Written from the behaviour that tests/golden/generator_trace.json pins (the reference's detikzify/infer/generate.py:145-353
executed on a scripted model; three reward modes: identical rollouts, scores, tree statistics, memo size and model calls),
not from its text.  What that behaviour is, in this file's terms:

  one expansion (`child_finder`, the callback detikzify_amd.mcts.MonteCarlo calls on the node it selected)
    1. CONTINUE the node's token prefix with the model and cut the stream into one tree position per source line
       (`rollout` -> `_LineCutter`); a position whose continuation is already known to fail takes that memoised tail and
       ends the generation on the spot (`_grow_chain`);
    2. a "widen" node re-rolls from its PARENT: count the visit, then skip the part of the chain the parent's subtree
       already holds (`merge`);
    3. COMPILE what the chain spells (`decode` -> document_class) and decide whether it can be rewarded at all
       (rasterisable, and — strict mode — free of errors);
    4. GRAFT: only round(sqrt(n)) of the n new positions enter the tree, as a single path (`_graft_path`).  A document
       that cannot be rewarded but names an error line keeps the positions BEFORE that line (same cap) and memoises the
       chain from the first position PAST it as a failing tail (`_graft_before_error`);
    5. REWARD the path's tip: SelfSim of the rendering (min-max normalised against every reward of this tree, lazily:
       infer/tree.DynMinMaxNorm), -1 when there is nothing to render; without a metric, compiler diagnostics
       (rewardable minus had-errors).  The (raw score, document) pair is what `simulate()` yields.

  generate()   early-out on EOS / the length budget, then model.generate with the image token banned and EOS suppressed
               at the first new position (reference :209-227 is the contract for these arguments)
  rollout()    generation in a background thread; the caller's thread receives the tokens one source line at a time

Departures that do not change results: the processor output of (image, text) is computed once per generator (or handed
in by simulate_parallel) instead of once per rollout; the newline table lives on the processor; the worker is a plain
thread, not a ThreadPool(1); streamed tokens arrive in line bursts (TokenStreamer(flush_on=...)).
The model object is detikzify_amd.model.DetikzifyForCausalLM (HIP); nothing here touches the GPU directly.
"""
from __future__ import annotations

import re
import threading
from collections import deque
from contextlib import nullcontext
from math import sqrt
from time import monotonic
from typing import Dict, Iterator, List, NamedTuple, Optional, Sequence, Tuple, Type

import torch
from PIL import Image

from ..mcts import MonteCarlo
from ..util import ExplicitAbort, StreamerList, TokenStreamer, cache_cast
from ..util import unwrap_processor as unwrap
from .tikz import TikzDocument
from .tree import DynMinMaxNorm, NodeState, Numeric, WideNode


class _BackgroundCall:
    """func(*args, **kwds) in one worker thread; an exception goes to error_callback; wait() joins.  What the reference
    gets from `ThreadPool(processes=1).apply_async(...)` + `pending.wait()` (infer/generate.py:248-258) without the pool's
    three housekeeping threads, whose start-up and 0.1 s polling cost 50-100 ms per rollout — nothing next to a LaTeX
    run, but a sixth of a rollout that is decoded in a 64-wide batch."""

    def __init__(self, func, args=(), kwds=None, error_callback=None):
        self._func, self._args, self._kwds, self._error_callback = func, args, kwds or {}, error_callback
        self.value = None
        self._thread = threading.Thread(target=self._run, name="detikzify-rollout", daemon=True)
        self._thread.start()

    def _run(self):
        try:
            self.value = self._func(*self._args, **self._kwds)
        except BaseException as e:  # noqa: BLE001  (forwarded: the consumer of the streamer must never wait forever)
            if self._error_callback is not None:
                self._error_callback(e)

    def wait(self, timeout: Optional[float] = None):
        self._thread.join(timeout)


class NewlineToken(NamedTuple):
    """what a vocabulary entry that contains line breaks does to the line count"""
    num_lines: int      # line breaks inside the token's text
    trailing: bool      # the text ENDS with one (otherwise the token already starts the next line)


def newline_table(processor) -> Dict[int, NewlineToken]:
    """token id -> NewlineToken for every vocabulary entry whose decoded text contains a line break (\\r\\n and \\r count as
    one).  Depends on the tokenizer alone, so it is kept on the (unwrapped) processor: the trees of simulate_parallel — one
    generator each — build it once, not once per tree (a vocabulary-sized loop of decode() calls under the tokenizer lock:
    HF fast tokenizers are not re-entrant)."""
    owner = unwrap(processor)
    with getattr(owner, "_tok_lock", nullcontext()):
        table = getattr(owner, "_newline_table", None)
        if table is None:
            table = {}
            for token_id in owner.tokenizer.vocab.values():
                text = re.sub(r"\r\n|\r", "\n", processor.decode([token_id]))
                breaks = text.count("\n")
                if breaks:
                    table[token_id] = NewlineToken(breaks, text.endswith("\n"))
            try:
                owner._newline_table = table
            except AttributeError:      # a processor type that forbids new attributes: per-generator table
                pass
    if not table:
        raise AssertionError("the vocabulary has no token with a line break: the search tree is built from source lines")
    return table


class _LineCutter:
    """Turns a token stream into tree positions, one per completed source line.

    A position is (all tokens up to and including the token that completed the line, number of lines so far).  A newline
    token that goes on with text after its last break has already begun the next line: that begun line is counted when the
    token arrives and taken back out of the NEXT newline token's count (and out of the final, unfinished position), so a
    line is never counted twice."""

    def __init__(self, prefix: torch.Tensor, num_lines: int, table: Dict[int, NewlineToken]):
        self.prefix, self.num_lines, self.table = prefix, num_lines, table
        self._open: List[int] = []          # tokens since the last completed line
        self._begun = 0                     # 1 while the last newline token spilled into a line that is still open

    def _take(self) -> torch.Tensor:
        self.prefix = torch.cat((self.prefix, torch.tensor(self._open, device=self.prefix.device)))
        self._open = []
        return self.prefix

    def push(self, token: int) -> Optional[Tuple[torch.Tensor, int]]:
        self._open.append(token)
        hit = self.table.get(token)
        if hit is None:
            return None
        self.num_lines += hit.num_lines - self._begun
        self._begun = 0 if hit.trailing else 1
        return self._take(), self.num_lines

    def rest(self) -> Optional[Tuple[torch.Tensor, int]]:
        """the unfinished last line, if the stream ended inside one"""
        if not self._open:
            return None
        return self._take(), self.num_lines - self._begun


class DetikzifyGenerator:
    def __init__(self, model, processor, image: Optional[Image.Image], text: Optional[str] = None,
                 metric=None, compile_timeout: Optional[int] = 60, mcts_timeout: Optional[int] = None,
                 streamer=None, control: Optional[ExplicitAbort] = None, exploration: float = 0.6,
                 strict: bool = False, document_class: Type[TikzDocument] = TikzDocument, processed=None, rng=None,
                 presence_penalty: Optional[float] = None, frequency_penalty: Optional[float] = None,
                 dry_multiplier: Optional[float] = None, dry_base: Optional[float] = None, dry_allowed_length: Optional[int] = None,
                 dry_sequence_breakers=None, min_new_tokens: Optional[int] = None, exponential_decay_length_penalty=None,
                 logit_bias=None, sequence_bias=None, top_logprobs: Optional[int] = None, prompt_lookup_rollouts: int = 0, **gen_kwargs):
        """prompt_lookup_rollouts=R (0 = off): with prompt_lookup_num_tokens on, the program part (the ids behind the root prompt) of the
        last R finished generate() results is passed to model.generate as prompt_lookup_corpus, newest first, behind the sequences of an
        explicit prompt_lookup_corpus= (tokenised boilerplate, say); the oldest are left out until model.generate's cap on the corpus
        holds.  Sibling rollouts share whole lines the new rollout's own history does not hold yet; the tokens are the same either way.
        top_logprobs=j (1 .. 8): every rollout of simulate() is generated with return_logprobs=True, top_logprobs=j, and every
        document it yields carries `.token_logprobs` / `.token_sample_logprobs` / `.token_top_ids` / `.token_top_logprobs`, one entry
        per token behind the prompt, as sample(return_logprobs=True, top_logprobs=j) attaches them.  Under a batch engine that needs an
        engine built with top_logprobs >= j (simulate_parallel builds it).
        presence_penalty / frequency_penalty (model.generate's; None / 0 = off): counted from the end of the image prompt on, so a
        rollout that continues a node of the tree penalises the whole program text so far, however its slot got there.
        min_new_tokens / exponential_decay_length_penalty (model.generate's) likewise count the program's tokens from the end of the
        image prompt (length_start); logit_bias / sequence_bias hold for every rollout"""
        if presence_penalty or frequency_penalty:
            gen_kwargs = {**gen_kwargs, "presence_penalty": presence_penalty, "frequency_penalty": frequency_penalty}
        if dry_multiplier:      # DRY (model.generate's) likewise: its history starts at the end of the image prompt
            gen_kwargs = {**gen_kwargs, "dry_multiplier": dry_multiplier, "dry_base": dry_base, "dry_allowed_length": dry_allowed_length,
                          "dry_sequence_breakers": dry_sequence_breakers}
        if min_new_tokens or exponential_decay_length_penalty is not None:      # length control (model.generate's): the program's length
            gen_kwargs = {**gen_kwargs, "min_new_tokens": min_new_tokens, "exponential_decay_length_penalty": exponential_decay_length_penalty}
        if logit_bias or sequence_bias:
            gen_kwargs = {**gen_kwargs, "logit_bias": logit_bias, "sequence_bias": sequence_bias}
        from ..model.modeling import check_top_logprobs
        self.top_logprobs = check_top_logprobs(top_logprobs)
        # the records of every token a rollout of this search produced, as a trie over the token sequences behind the root: a rollout
        # continues a node of an earlier one, so a document's records come from several calls.  (parent entry, token) -> entry;
        # _records[entry] = (logprob, sample_logprob, top ids, top logprobs).  It grows by one entry per token a rollout produces and is
        # never pruned: it lives as long as the search, like the tree itself (some hundred bytes per token)
        self._record_at: Dict[Tuple[int, int], int] = {}
        self._records: List[Tuple[float, float, List[int], List[float]]] = [(float("nan"), float("nan"), [], [])]      # entry 0: the root
        self._records_lock = threading.Lock()
        self.model, self.processor = model, processor
        self.image, self.text, self.metric = image, text, metric
        self.compile_timeout, self.mcts_timeout = compile_timeout, mcts_timeout
        self.streamer, self.control = streamer, control or ExplicitAbort()
        self.exploration, self.strict, self.document_class = exploration, strict, document_class
        self.gen_kwargs = gen_kwargs
        if isinstance(prompt_lookup_rollouts, bool) or not isinstance(prompt_lookup_rollouts, int) or prompt_lookup_rollouts < 0:
            raise ValueError(f"prompt_lookup_rollouts = {prompt_lookup_rollouts!r}: a number of rollouts >= 0")
        self.prompt_lookup_rollouts = prompt_lookup_rollouts
        self._rollouts: deque = deque(maxlen=prompt_lookup_rollouts or None)      # program parts of the last R results, oldest first
        self._rollouts_lock = threading.Lock()
        # processor output of (image, text) — the AdapterProcessor's for a text — built on first use unless handed in (the trees of
        # simulate_parallel share one)
        self._processed = processed
        self._newlines: Optional[Dict[int, NewlineToken]] = None

        self.norm = DynMinMaxNorm()
        self.failed_rollouts: Dict[NodeState, List[WideNode]] = {}      # position -> the chain that failed from there on
        self.solution: deque = deque(maxlen=1)                          # the last expansion's (score, document)
        prompt = processed if processed is not None else processor(images=image, text=text, return_tensors="pt")
        # rng: this tree's own random.Random for the search's tie-breaks (parallel trees); None = the module-level stream, as the reference
        self.montecarlo = MonteCarlo(root_node=self._node(prompt.input_ids.to(model.device).squeeze(), 0), rng=rng)
        self.montecarlo.child_finder = self.child_finder
        # equal token sequences decode to the SAME document object and equal renderings score once (the search revisits
        # positions; a TikzDocument compiles lazily and keeps its result)
        by_tokens, by_pixels = cache_cast(lambda ids: tuple(ids.tolist())), cache_cast(lambda rendering: rendering.tobytes())
        self.decode, self.score = by_tokens(self.decode), by_pixels(self.score)

    def _node(self, token_ids: torch.Tensor, num_lines: int) -> WideNode:
        return WideNode(token_ids, num_lines, exploration=self.exploration)

    @property
    def newlineinfo(self) -> Dict[int, NewlineToken]:
        if self._newlines is None:
            self._newlines = newline_table(self.processor)
        return self._newlines

    # ---- front-end -------------------------------------------------------------------------------------------------
    def simulate(self, expansions: Optional[Numeric] = 1) -> Iterator[Tuple[Numeric, TikzDocument]]:
        """one MCTS expansion per item: (score, document) of its rollout.  `expansions=None` runs until `mcts_timeout`
        (checked after an expansion: the budget never cuts a rollout short, at least one is always produced)."""
        deadline = None if self.mcts_timeout is None else monotonic() + self.mcts_timeout
        done = 0
        while expansions is None or done < expansions:
            self.montecarlo.simulate()
            done += 1
            yield self.solution.pop()
            if deadline is not None and monotonic() > deadline:
                break

    __call__ = simulate         # a generator object is callable like its simulate()

    def sample(self, return_logprobs: bool = False, top_logprobs: Optional[int] = None) -> TikzDocument:
        """return_logprobs: the document carries `.token_logprobs` / `.token_sample_logprobs`, one float per generated token (EOS
        included): the model's log-probability of the token and the log of the probability the sampler drew it with.  top_logprobs=k
        (with return_logprobs): + `.token_top_ids` / `.token_top_logprobs`, per generated token the k most likely tokens at its position"""
        from ..model.modeling import check_top_logprobs
        topk = check_top_logprobs(top_logprobs, return_logprobs)
        if not return_logprobs:
            return self.decode(self.generate(input_ids=self.montecarlo.root_node.token_ids))
        out = self.generate(input_ids=self.montecarlo.root_node.token_ids, return_logprobs=True, **({"top_logprobs": topk} if topk else {}))
        if not hasattr(out, "sequences"):       # self.generate returned the prompt itself, without a model call (it ends in EOS / fills the budget)
            document = self.decode(out)
            document.token_logprobs, document.token_sample_logprobs = [], []
            if topk:
                document.token_top_ids, document.token_top_logprobs = [], []
            return document
        document = self.decode(out.sequences.squeeze(0))
        document.token_logprobs = [float(v) for v in out.logprobs[0]]
        document.token_sample_logprobs = [float(v) for v in out.sample_logprobs[0]]
        if topk:
            document.token_top_ids = [[int(v) for v in row] for row in out.top_ids[0]]
            document.token_top_logprobs = [[float(v) for v in row] for row in out.top_logprobs[0]]
        return document

    # ---- a·G: one call of the model ------------------------------------------------------------------------------------
    def _prompt_features(self):
        if self._processed is None:
            self._processed = self.processor(images=self.image, text=self.text, text_kwargs={"truncation": True},
                                             return_tensors="pt")
        return self._processed

    def _negative_features(self, negative_image: Optional[Image.Image], negative_text: Optional[str]) -> Dict[str, torch.Tensor]:
        """the negative branch of a guided rollout (model.generate's guidance_scale) as model.generate's arguments: the negative image
        through the same processor (default: a white canvas of the processor's size), the negative text through the adapter's
        tokenizer.  A text-only prompt needs a negative text: the adapter's dummy input cannot be prefilled without one.  Built once
        per (image, text)"""
        key = (id(negative_image), negative_text)
        cached = getattr(self, "_negative", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        if self.image is None and negative_text is None:
            raise ValueError("guidance_scale with a text-only prompt needs negative_text: the negative branch is the adapter's dummy input "
                             "under another text (it cannot be prefilled without one)")
        out: Dict[str, torch.Tensor] = {}
        if self.image is not None:
            if negative_image is None:
                size = getattr(getattr(unwrap(self.processor), "image_processor", None), "size", None) or {}
                w, h = (size["width"], size["height"]) if "width" in size and "height" in size else self.image.size
                negative_image = Image.new("RGB", (int(w), int(h)), color="white")
            feats = self.processor(images=negative_image, return_tensors="pt", **({"text": negative_text} if negative_text is not None else {}))
            out["negative_pixel_values"] = feats["pixel_values"]
        else:
            feats = self.processor(text=negative_text, return_tensors="pt")
        if negative_text is not None:
            if "adapter_input_ids" not in feats:
                raise ValueError("negative_text needs the adapter's processor (a model loaded with adapter=True)")
            out["negative_adapter_input_ids"] = feats["adapter_input_ids"]
        self._negative = (key, out)
        return out

    def generate(self, input_ids: torch.Tensor, streamer=None, **gen_kwargs) -> torch.Tensor:
        sinks = StreamerList([s for s in (streamer, self.streamer) if s])
        options = {**self.gen_kwargs, **gen_kwargs}
        # classifier-free guidance (model.generate's guidance_scale): negative_image / negative_text become the negative branch's tensors
        negative_image, negative_text = options.pop("negative_image", None), options.pop("negative_text", None)
        from ..model.modeling import check_guidance_scale
        guided = check_guidance_scale(options.get("guidance_scale")) != 1.0
        if (options.get("presence_penalty") or options.get("frequency_penalty")) and options.get("penalty_start") is None:
            options["penalty_start"] = int(self.montecarlo.root_node.token_ids.numel())       # the program text so far counts, the prompt does not
        if options.get("dry_multiplier") and options.get("dry_start") is None:
            options["dry_start"] = int(self.montecarlo.root_node.token_ids.numel())           # likewise: a rollout sees the whole program text so far
        if (options.get("min_new_tokens") or options.get("exponential_decay_length_penalty") is not None) and options.get("length_start") is None:
            options["length_start"] = int(self.montecarlo.root_node.token_ids.numel())        # likewise: the whole program's length counts
        budget = options.get("max_length", self.model.generation_config.to_dict().get("max_length"))
        n = input_ids.numel()
        finished = n > 0 and input_ids[-1] == unwrap(self.processor).tokenizer.eos_token_id
        if finished or n >= budget:         # nothing may follow EOS, nothing fits beyond the budget
            sinks.end()
            return input_ids
        keep = bool(self.prompt_lookup_rollouts and options.get("prompt_lookup_num_tokens"))
        if keep:
            corpus = self._lookup_corpus(options.get("prompt_lookup_corpus"))
            if corpus:
                options["prompt_lookup_corpus"] = corpus
        with torch.inference_mode():
            features = self._prompt_features().to(self.model.device)
            conditioning = {name: value for name, value in features.items() if name.startswith("adapter")}
            if guided:
                conditioning.update({name: value.to(self.model.device) for name, value in self._negative_features(negative_image, negative_text).items()})
            out = self.model.generate(
                input_ids=input_ids[None],
                pixel_values=features.get("pixel_values"),
                bad_words_ids=[[self.model.config.image_token_id]],                     # never emit the image placeholder
                begin_suppress_tokens=[self.model.config.text_config.eos_token_id],     # never an empty program
                streamer=sinks,
                **conditioning, **options)
        if keep:      # the program part of a finished result: a later rollout of this image drafts from it
            seq = (out.sequences if hasattr(out, "sequences") else out).reshape(-1)
            program = [int(t) for t in seq[int(self.montecarlo.root_node.token_ids.numel()):]]
            if program:
                with self._rollouts_lock:
                    self._rollouts.append(program)
        return out if hasattr(out, "sequences") else out.squeeze()      # (return_logprobs=True: the GenerateOutput as it is)

    def _lookup_corpus(self, explicit) -> List[List[int]]:
        """model.generate's prompt_lookup_corpus: the caller's own sequences first, then the kept rollouts, newest first; the oldest
        rollouts are left out until the ids and one separator between sequences fit the cap (the caller's sequences are never cut:
        model.generate refuses them if they alone exceed it)"""
        from .. import _lib
        first = [s for s in ([t.tolist() if isinstance(t, torch.Tensor) else list(t) for t in explicit] if explicit is not None else []) if s]
        with self._rollouts_lock:
            kept = list(self._rollouts)[::-1]
        room = _lib.DTK_SPEC_CORPUS_MAX - (sum(len(s) for s in first) + max(0, len(first) - 1))
        out = list(first)
        for program in kept:
            cost = len(program) + (1 if out else 0)
            if cost > room:
                break
            out.append(program)
            room -= cost
        return out

    def _generate_recorded(self, input_ids: torch.Tensor, **kw) -> torch.Tensor:
        """generate() of a rollout under top_logprobs: the same tokens, and the new tokens' records filed under their sequence"""
        out = self.generate(input_ids, return_logprobs=True, top_logprobs=self.top_logprobs, **kw)
        if not hasattr(out, "sequences"):       # the prompt itself came back, without a model call
            return out
        seq = out.sequences.reshape(-1)
        result = out.sequences.squeeze()      # what generate() returns for a plain call
        n0, root = int(input_ids.numel()), int(self.montecarlo.root_node.token_ids.numel())
        toks = [int(t) for t in seq[root:]]
        with self._records_lock:
            at = 0
            for i, tok in enumerate(toks):
                nxt = self._record_at.get((at, tok))
                new = root + i - n0        # index among this call's new tokens (< 0: a token of the node the rollout continued)
                if nxt is None:
                    nxt = len(self._records)
                    self._record_at[(at, tok)] = nxt
                    self._records.append((float("nan"), float("nan"), [-1] * self.top_logprobs, [float("nan")] * self.top_logprobs))
                if new >= 0:
                    self._records[nxt] = (float(out.logprobs[0, new]), float(out.sample_logprobs[0, new]),
                                          [int(v) for v in out.top_ids[0, new]], [float(v) for v in out.top_logprobs[0, new]])
                at = nxt
        return result

    def _attach_records(self, document: TikzDocument, token_ids: torch.Tensor) -> None:
        """top_logprobs: the four per-token lists of `document`, whose tokens are token_ids behind the root"""
        root = int(self.montecarlo.root_node.token_ids.numel())
        nan = (float("nan"), float("nan"), [-1] * self.top_logprobs, [float("nan")] * self.top_logprobs)
        rows, at = [], 0
        with self._records_lock:
            for tok in token_ids.reshape(-1)[root:].tolist():
                at = self._record_at.get((at, int(tok)), -1) if at >= 0 else -1
                rows.append(self._records[at] if at >= 0 else nan)
        document.token_logprobs = [r[0] for r in rows]
        document.token_sample_logprobs = [r[1] for r in rows]
        document.token_top_ids = [list(r[2]) for r in rows]
        document.token_top_logprobs = [list(r[3]) for r in rows]

    # ---- a·R: a generation as a stream of tree positions -------------------------------------------------------------------
    def rollout(self, state: NodeState) -> Iterator[Tuple[torch.Tensor, int]]:
        """continue `state` to the end in a worker thread; yields (token prefix, #lines) after every completed source line
        (and once more for an unfinished last line).  Closing the iterator aborts the generation; an abort from elsewhere
        (`control.abort()`) surfaces as InterruptedError after the stream has ended."""
        table = self.newlineinfo
        cutter = _LineCutter(state.token_ids, state.num_lines, table)
        tokens = TokenStreamer(flush_on=table)       # same tokens, handed over one source line at a time
        worker = _BackgroundCall(self._generate_recorded if self.top_logprobs else self.generate, args=[state.token_ids], error_callback=tokens.propagate_error,
                                 kwds=dict(stopping_criteria=[self.control.reset()], streamer=tokens))
        try:
            for token in tokens:
                position = cutter.push(token)
                if position is not None:
                    yield position
            tail = cutter.rest()
            if tail is not None:
                yield tail
            if self.control.should_stop:
                raise InterruptedError
        except (GeneratorExit, KeyboardInterrupt):
            self.control.abort()
            raise
        finally:
            worker.wait()

    def decode(self, token_ids: torch.Tensor) -> TikzDocument:
        new_tokens = token_ids[len(self.montecarlo.root_node.token_ids):]
        return self.document_class(code=self.processor.decode(new_tokens, skip_special_tokens=True), timeout=self.compile_timeout)

    def score(self, image: Image.Image) -> Numeric:
        assert self.metric
        self.metric.update(img1=image, img2=self.image, text2=self.text)
        try:
            return self.metric.compute()
        finally:
            self.metric.reset()

    # ---- a·M: one expansion ----------------------------------------------------------------------------------------------
    def _grow_chain(self, start: NodeState) -> List[WideNode]:
        """the new positions of one rollout from `start`, oldest first"""
        chain: List[WideNode] = []
        stream = self.rollout(start)
        for token_ids, num_lines in stream:
            fresh = self._node(token_ids, num_lines)
            known_tail = self.failed_rollouts.get(fresh.state)
            if known_tail is not None:      # this position is known to end in a failure: reuse that ending, stop generating
                chain += known_tail
                stream.close()
                break
            chain.append(fresh)
        return chain

    def merge(self, node: WideNode, nodes_to_merge: Sequence[WideNode]) -> Tuple[WideNode, List[WideNode]]:
        """descend from `node` along children that hold the same positions as the head of the chain; returns where the
        descent ended and the part of the chain that is new there"""
        taken = 0
        while taken < len(nodes_to_merge):
            wanted = nodes_to_merge[taken].state
            twin = next((child for child in node.children if child.state == wanted), None)
            if twin is None:
                break
            node, taken = twin, taken + 1
        return node, list(nodes_to_merge[taken:])

    @staticmethod
    def _graft_path(anchor: WideNode, path: Sequence[WideNode]) -> WideNode:
        for link in path:
            anchor.add_child(link)
            anchor = link
        return anchor

    def _graft_before_error(self, anchor: WideNode, chain: List[WideNode], cap: int, error_line: int) -> WideNode:
        """positions in front of the first located error join the tree (at most `cap`: those with index < cap); the chain
        from the first position beyond the error line is remembered as a failing continuation of that position.  A position
        whose last line IS the error line is neither (the line may still be incomplete).

        Deliberately bug-for-bug: the reference has one more branch here — `num_lines == errorln and ends_with_eol` memoises the
        failing tail from the error line itself (detikzify/infer/generate.py:331-336) — but it looks the line ending up with
        `self.newlineinfo.get(<0-d tensor>)`, tensors hash by identity, so the lookup always misses and the branch is never
        taken.  This port keeps what the reference DOES (and what tests/golden/generator_trace.json records), not what it
        intends; if upstream fixes the lookup, add `or (link.num_lines == error_line and <last token ends with a newline>)` to
        the first test below and regenerate the golden trace."""
        for i, link in enumerate(chain):
            if link.num_lines > error_line:
                self.failed_rollouts[link.state] = chain[i:]
                break
            if link.num_lines < error_line and i < cap:
                anchor.add_child(link)
                anchor = link
        return anchor

    def child_finder(self, node: WideNode, montecarlo: MonteCarlo) -> None:
        chain = self._grow_chain(node.state)
        if node.is_widen_node:              # a re-roll at the parent's position: it is the parent that grows
            node.visits += 1
            node, chain = self.merge(node.parent, chain)

        document = self.decode(chain[-1].token_ids if chain else node.token_ids)
        if self.top_logprobs:
            self._attach_records(document, chain[-1].token_ids if chain else node.token_ids)
        cap = round(sqrt(len(chain)))       # sqrt(n) of n new lines enter the tree
        rewardable = bool(document.is_rasterizable) and not (self.strict and document.compiled_with_errors)

        if rewardable:
            tip = self._graft_path(node, chain[:cap])
        else:
            first_error = min(document.errors or [0])       # 0: nothing located (errors are keyed by 1-based line)
            tip = self._graft_before_error(node, chain, cap, first_error) if first_error else node

        if self.metric:
            score = self.score(document.rasterize()) if rewardable else -1
            tip.update_win_value(self.norm(score) if rewardable else score)
        else:       # compiler diagnostics as the reward: 1 clean, 0 rendered with errors / not rendered but error-free, -1 failed
            score = rewardable - document.compiled_with_errors
            tip.update_win_value(score)
        self.solution.append((score, document))


# the name BASELINE.json's north_star uses for the drop-in
TikzGenerator = DetikzifyGenerator
