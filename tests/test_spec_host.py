"""Prompt-lookup speculative decoding, host side (no GPU): the lookup rule against a brute-force restatement, the additive C ABI, the
argument checks and refusals of generate() — which run before any library call — and the loop of a speculative generate() on a
scripted device: slot 0, the pipelining, one token at a time to the streamer, the stop inside an accepted run, spec_end's length."""
import random
import re
from pathlib import Path

import pytest
import torch

from detikzify_amd import _lib
from detikzify_amd.infer.batching import BatchEngine
from detikzify_amd.infer.generate import DetikzifyGenerator
from detikzify_amd.model.modeling import GenerateOutput, check_prompt_lookup

from . import spec_oracle
from .helpers import FakeModel, fake_processor, sketch_image
from .test_generate_loop import EOS, IMG, NIMG, VOCAB, ScriptedDevice, _prompt

NEW = ("dtk_spec_begin", "dtk_spec_set_drafts", "dtk_spec_launch", "dtk_spec_wait", "dtk_spec_end", "dtk_op_spec_lookup", "dtk_bench_spec")
GEN = dict(bad_words_ids=[[IMG]], begin_suppress_tokens=[EOS], do_sample=True, seed=7)


# ------------------------------------------------------------------------------------------ the lookup rule
def test_lookup_on_the_named_cases():
    look = spec_oracle.lookup
    assert look([], 3, 2) == [] and look([5], 3, 2) == []                        # empty and one-id histories
    assert look([7, 7, 7, 7], 3, 2) == [7, 7]                                     # a a a a: window 0 matches (7, 7), two ids follow it
    assert look([7, 7, 7, 7], 1, 2) == [7] and look([7, 7, 7, 7], 3, 1) == [7, 7, 7]
    assert look([1, 2, 3, 9, 1, 2], 3, 2) == [3, 9, 1]                            # the continuation of the earlier (1, 2)
    assert look([4, 1, 2], 3, 1) == [] and look([1, 2, 3], 3, 2) == []           # no earlier occurrence
    assert look([8, 1, 2, 5, 1, 2], 3, 2) == [5, 1, 2]
    assert look([9, 9, 1, 2, 1, 2], 3, 2) == [1, 2]                               # a match whose continuation is cut by the end
    # a longer n-gram beats an earlier shorter one: (2) alone first occurs at index 0, (1, 2) at index 3
    assert look([2, 6, 6, 1, 2, 4, 1, 2], 2, 2) == [4, 1] and look([2, 6, 6, 1, 2, 4, 1, 2], 2, 1) == [6, 6]
    # the cut at max_positions: the last id sits at position len - 1, no draft's position may reach max_positions
    ids = [1, 2, 3, 4, 1, 2]
    assert look(ids, 3, 2, max_positions=9) == [3, 4, 1] and look(ids, 3, 2, max_positions=8) == [3, 4]
    assert look(ids, 3, 2, max_positions=7) == [3] and look(ids, 3, 2, max_positions=6) == []


def test_lookup_equals_the_brute_force_restatement():
    rng = random.Random(5)
    n = 0
    for alphabet in (2, 3, 6, 50):
        for L in list(range(0, 12)) + [17, 40, 65]:
            for _ in range(6):
                ids = [rng.randrange(alphabet) for _ in range(L)]
                for K in (1, 2, 3):
                    for ng in (1, 2, 3, 4):
                        for cap in (None, L, L + 1, L + 2, L + 7):
                            assert spec_oracle.lookup(ids, K, ng, cap) == spec_oracle.lookup_brute(ids, K, ng, cap), (ids, K, ng, cap)
                            n += 1
    assert n > 10000


def test_accept_pattern_ends_runs_at_the_corrupted_positions():
    T, K = 10, 3
    seq = list(range(100, 160))
    table = [-1] * T + seq[T:]
    assert spec_oracle.accept_pattern(seq, table, T, K, 9, 2048) == [1, 4, 4]      # all right: K + 1 per step behind the first
    wrong = [-1] * T + [t + 1 for t in seq[T:]]
    assert spec_oracle.accept_pattern(seq, wrong, T, K, 5, 2048) == [1] * 5         # all wrong: one token per step
    bad = list(table)
    bad[T + 3] += 1                                                                 # the run that reaches position T + 3 ends there
    assert spec_oracle.accept_pattern(seq, bad, T, K, 9, 2048) == [1, 3, 4, 4]
    holes = list(table)
    holes[T + 2] = -1                                                               # no draft at a position: the step carries one draft, and its
    assert spec_oracle.accept_pattern(seq, holes, T, K, 9, 2048) == [1, 2, 4, 4]    # free token is the one at the hole


# ------------------------------------------------------------------------------------------ the C ABI
def test_abi_is_additive():
    header = (Path(__file__).resolve().parents[1] / "include" / "dtk.h").read_text()
    lib = _lib.load_library()
    assert re.search(r"^#define DTK_ABI_VERSION 7\b", header, re.M) and lib.dtk_abi_version() == 7 == _lib.DTK_ABI_VERSION
    for name in NEW:
        decl = re.search(rf"^int\s+{name}\((.*?)\);", header, re.M | re.S)
        assert decl, f"{name} is not declared in dtk.h"
        assert name in _lib.SYMBOLS and getattr(lib, name).argtypes is not None
        assert len(_lib.SYMBOLS[name][1]) == decl.group(1).count(",") + 1, name
    assert re.search(r"#define\s+DTK_SPEC_MAX_NGRAM\s+%d\b" % _lib.DTK_SPEC_MAX_NGRAM, header)
    assert re.search(r"DTK_SPEC_LOOKUP = %d, DTK_SPEC_TABLE = %d" % (_lib.DTK_SPEC_LOOKUP, _lib.DTK_SPEC_TABLE), header)


# ------------------------------------------------------------------------------------------ generate(): checks and refusals
class SpecDevice(ScriptedDevice):
    """ScriptedDevice with the speculative wrappers: a step accepts 1 .. K + 1 of the toy LM's next tokens (the count a function of the
    length), so the sequence is the plain one whatever is accepted"""

    def __init__(self, slots=0, **kw):
        super().__init__(slots=slots, **kw)
        self.calls, self.spending, self.spec, self.kept = [], [], None, None

    def set_sampling(self, *a, **kw):
        self.calls.append(("set_sampling", kw.get("slot")))
        super().set_sampling(*a, **kw)

    def prefill(self, input_ids, pixel_values=None, **kw):
        self.calls.append(("prefill", kw.get("slot")))
        super().prefill(input_ids, pixel_values, **kw)

    def decode_launch(self):
        self.calls.append(("decode_launch",))
        super().decode_launch()

    def spec_begin(self, num_tokens, max_ngram=2, table=False):
        assert self.spec is None and 0 in self.ctx
        self.calls.append(("spec_begin", num_tokens, max_ngram, table))
        self.spec = num_tokens

    def spec_set_drafts(self, table):
        self.calls.append(("spec_set_drafts", len(table)))

    def spec_launch(self):
        assert self.spec and len(self.spending) < 2
        known = len(self.ctx[0]) - sum(len(s) for s in self.spending)
        assert known + 4 * len(self.spending) < self.config.max_positions, "a launch the library would refuse (DTK_ERR_RANGE)"
        n = 1 + (len(self.ctx[0]) * 7 + 3) % (self.spec + 1)
        n = min(n, self.config.max_positions - len(self.ctx[0]))
        self.spending.append([self._next(0) for _ in range(n)])
        self.calls.append(("spec_launch",))

    def spec_wait(self, logprobs=False):
        assert not logprobs
        return self.spending.pop(0)

    def spec_end(self, keep_len):
        self.calls.append(("spec_end", keep_len))
        self.spending.clear()
        self.ctx[0], self.spec, self.kept = self.ctx[0][:keep_len], None, keep_len


@pytest.mark.parametrize("k, n", [(-1, None), (4, None), (True, None), (1.5, None), ("2", None), (2, 0), (2, 17), (2, True), (2, 1.0), (None, 0)])
def test_bad_values_raise_before_any_call(k, n):
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens|max_matching_ngram_size"):
        check_prompt_lookup(k, n)
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0)
    dev = SpecDevice(slots=5)
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens|max_matching_ngram_size"):
        dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=4, prompt_lookup_num_tokens=k, max_matching_ngram_size=n, **GEN)
    assert dev.calls == []
    dev.generation_config.prompt_lookup_num_tokens, dev.generation_config.max_matching_ngram_size = k, n
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens|max_matching_ngram_size"):
        dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=4, **GEN)
    assert dev.calls == []


def test_check_returns_hf_defaults():
    assert check_prompt_lookup(None) == (0, 2) and check_prompt_lookup(0, 3) == (0, 3)
    assert check_prompt_lookup(3) == (3, 2) and check_prompt_lookup(1, 16) == (1, 16)


@pytest.mark.parametrize("k", [None, 0])
def test_off_makes_the_calls_of_a_plain_generate(k):
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0)
    plain, dev = SpecDevice(slots=5), SpecDevice(slots=5)
    want = plain.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=12, **GEN)
    got = dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=12, prompt_lookup_num_tokens=k, **GEN)
    assert torch.equal(got, want) and dev.calls == plain.calls
    assert all(c[0] in ("set_sampling", "prefill", "decode_launch") and (len(c) < 2 or c[1] is None) for c in dev.calls)
    # a fake without the speculative wrappers keeps working with the argument off
    bare = ScriptedDevice()
    assert torch.equal(bare.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=12, prompt_lookup_num_tokens=k, **GEN), want)


def test_refusals_name_the_argument_and_touch_nothing():
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0)
    call = dict(input_ids=ids[None], pixel_values=px, max_new_tokens=4, **GEN)
    for slots, k in ((0, 1), (1, 1), (2, 2), (3, 3)):        # fewer than K + 1 slots: the load(...) hint, as guidance_scale
        small = SpecDevice(slots=slots)
        with pytest.raises(ValueError, match=r"batch_slots=%d" % (k + 1)):
            small.generate(prompt_lookup_num_tokens=k, **call)
        assert small.calls == []
    dev = SpecDevice(slots=5)
    for extra in (dict(guidance_scale=2.0, negative_pixel_values=px * 0), dict(presence_penalty=0.5), dict(frequency_penalty=0.5),
                  dict(dry_multiplier=0.8), dict(min_new_tokens=3), dict(exponential_decay_length_penalty=(2, 1.1)),
                  dict(logit_bias={5: 1.0}), dict(return_logprobs=True, top_logprobs=2)):
        with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens"):
            dev.generate(prompt_lookup_num_tokens=2, **call, **extra)
        assert dev.calls == []
    wide = SpecDevice(slots=16)          # outside the multi-vector family
    with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens.*16 batch slots"):
        wide.generate(prompt_lookup_num_tokens=2, **call)
    assert wide.calls == []
    dev.config.kv_format = "mxfp8"
    with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens.*mxfp8"):
        dev.generate(prompt_lookup_num_tokens=2, **call)
    dev.config.kv_format = "bf16"
    with pytest.raises(ValueError, match="prompt_lookup_drafts without"):
        dev.generate(prompt_lookup_drafts=[1, 2, 3], **call)
    eng = BatchEngine(dev, max_batch=4)
    try:
        seen = []
        eng.sequence = lambda *a, **k: seen.append(a) or (_ for _ in ()).throw(AssertionError("the engine saw a sequence"))
        with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens: not in the batch engines"):
            dev.generate(prompt_lookup_num_tokens=2, **call)
        assert seen == []
    finally:
        del eng.sequence
        eng.close()
    assert dev.calls == []


# ------------------------------------------------------------------------------------------ generate(): the loop
class _Recorder:
    def __init__(self):
        self.events = []

    def put(self, value):
        self.events.append(value.reshape(-1).tolist())

    def end(self):
        self.events.append("end")


@pytest.mark.parametrize("k", [1, 2, 3])
def test_loop_of_a_speculative_generate(k):
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0, extra=[40, 41])
    T = ids.numel()
    plain, dev = SpecDevice(slots=5), SpecDevice(slots=5)
    free = dict(suppress_tokens=[EOS], eos_token_id=-1)
    want = plain.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=25, **GEN, **free)
    rec = _Recorder()
    got = dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=25, prompt_lookup_num_tokens=k, max_matching_ngram_size=3,
                       streamer=rec, **GEN, **free)
    assert torch.equal(got, want) and got.shape == (1, T + 25)
    assert rec.events[0] == ids.tolist() and rec.events[-1] == "end" and rec.events[1:-1] == [[t] for t in got[0, T:].tolist()]
    names = [c[0] for c in dev.calls]
    assert dev.calls[0] == ("set_sampling", 0) and dev.calls[1] == ("prefill", 0) and dev.calls[2] == ("spec_begin", k, 3, False)
    assert "decode_launch" not in names and "spec_set_drafts" not in names
    assert dev.calls[-1] == ("spec_end", T + 25) and dev.ctx[0] == got[0].tolist() and dev.spec is None      # the slot holds the output exactly
    assert 25 / (k + 1) <= names.count("spec_launch") <= 26


def test_stop_inside_an_accepted_run_and_the_context_end():
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0, extra=[40, 41])
    T = ids.numel()
    plain = SpecDevice(slots=5)
    want = plain.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=30, **GEN, suppress_tokens=[EOS], eos_token_id=-1)
    new = want[0, T:].tolist()
    # an id that falls in the middle of a step's tokens ends the sequence there: the rest of the step is dropped
    dev = SpecDevice(slots=5)
    out = dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=30, prompt_lookup_num_tokens=3, return_logprobs=False,
                       **GEN, suppress_tokens=[EOS], eos_token_id=new[6])
    cut = new.index(new[6]) + 1
    assert out[0, T:].tolist() == new[:cut] and dev.calls[-1] == ("spec_end", T + cut) and dev.ctx[0] == out[0].tolist()
    # the context end: the loop never launches what the library would refuse, and fills the context exactly
    small = SpecDevice(slots=5, max_positions=T + 9)
    full = small.generate(input_ids=ids[None], pixel_values=px, max_length=10 ** 6, prompt_lookup_num_tokens=3, **GEN, suppress_tokens=[EOS],
                          eos_token_id=-1)
    assert full[0, T:].tolist() == new[:9] and small.calls[-1] == ("spec_end", T + 9)


def test_a_consumer_that_quits_still_ends_the_speculation():
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0)

    class Quits(_Recorder):
        def put(self, value):
            super().put(value)
            if len(self.events) == 4:
                raise RuntimeError("consumer gone")

    dev = SpecDevice(slots=5)
    with pytest.raises(RuntimeError, match="consumer gone"):
        dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=20, prompt_lookup_num_tokens=2, streamer=Quits(), **GEN)
    assert dev.calls[-1][0] == "spec_end" and dev.spec is None and not dev._single_busy.locked()


def test_drafts_table_and_output_record():
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0)
    dev = SpecDevice(slots=5)
    dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=5, prompt_lookup_num_tokens=2, prompt_lookup_drafts=[-1] * 40, **GEN)
    assert ("spec_begin", 2, 2, True) in dev.calls and ("spec_set_drafts", 40) in dev.calls
    assert dev.calls.index(("spec_set_drafts", 40)) == dev.calls.index(("spec_begin", 2, 2, True)) + 1
    out = GenerateOutput(torch.zeros(1, 3), torch.zeros(1, 0), torch.zeros(1, 0))
    assert out.accepted_per_step is None


def test_generator_and_pipeline_pass_the_arguments_through():
    seen = []

    class Model(FakeModel):
        def generate(self, **kw):
            seen.append({k: kw[k] for k in ("prompt_lookup_num_tokens", "max_matching_ngram_size") if k in kw})
            return super().generate(**{k: v for k, v in kw.items() if k not in ("prompt_lookup_num_tokens", "max_matching_ngram_size")})

    proc = fake_processor(512, 12)
    gen = DetikzifyGenerator(Model(), proc, sketch_image(1, 96), prompt_lookup_num_tokens=3, max_matching_ngram_size=2, max_length=30)
    gen.sample()
    assert seen and seen[0] == dict(prompt_lookup_num_tokens=3, max_matching_ngram_size=2)
    from detikzify_amd.infer.pipeline import DetikzifyPipeline
    seen.clear()
    pipe = DetikzifyPipeline(Model(), proc, metric="fast", prompt_lookup_num_tokens=2, max_length=30)
    pipe.sample(sketch_image(1, 96))
    next(iter(pipe.simulate(sketch_image(1, 96), expansions=1)))
    assert len(seen) >= 2 and all(s == dict(prompt_lookup_num_tokens=2) for s in seen)
