"""Prompt-lookup drafting from a corpus of earlier programs, host side (no GPU): the kernels' single-pass formulation against the
nested loops of the rule, the known answers, the additive C ABI, the argument checks of generate(), the life of the corpus around a
speculative generate() on a scripted device, and the corpus DetikzifyGenerator builds from its last rollouts."""
import random
import re
from pathlib import Path

import pytest
import torch

from detikzify_amd import _lib
from detikzify_amd.infer.generate import DetikzifyGenerator
from detikzify_amd.model.modeling import GenerateOutput, flatten_corpus

from . import spec_corpus_oracle as oracle
from . import spec_oracle
from .helpers import FakeModel, fake_processor, sketch_image
from .test_generate_loop import NIMG, VOCAB, ScriptedDevice, _prompt
from .test_spec_host import GEN, SpecDevice

NONE, HISTORY, CORPUS = oracle.NONE, oracle.HISTORY, oracle.CORPUS
NEW = ("dtk_spec_set_corpus", "dtk_spec_corpus_len", "dtk_spec_counters", "dtk_op_spec_lookup_corpus")

# (history, corpus, K, max_ngram, max_positions) -> (drafts, source, n): shared with the device test
KNOWN = [
    # own history wins at equal n: (1, 2) occurs in both, the history's continuation is taken
    (([1, 2, 7, 8, 1, 2], [1, 2, 5, 6], 3, 2, None), ([7, 8, 1], HISTORY, 2)),
    # a longer corpus n beats a shorter own n: the history matches (2) alone, the corpus (1, 2)
    (([2, 9, 1, 2], [4, 1, 2, 5, 6, 3], 3, 2, None), ([5, 6, 3], CORPUS, 2)),
    (([2, 9, 1, 2], [4, 1, 2, 5, 6, 3], 3, 1, None), ([9, 1, 2], HISTORY, 1)),
    # a separator inside a window: 1 | 2 is no occurrence of (1, 2); n = 1 then finds 2 in the history
    (([3, 1, 2], [1, -1, 2, 5], 3, 2, None), ([5], CORPUS, 1)),
    (([2, 3, 1, 2], [1, -1, 2, 5], 3, 2, None), ([3, 1, 2], HISTORY, 1)),
    # a continuation cut by a separator, and by the corpus end
    (([9, 1, 2], [1, 2, 5, -1, 6, 7], 3, 2, None), ([5], CORPUS, 2)),
    (([9, 1, 2], [8, 8, 1, 2, 5, 6], 3, 2, None), ([5, 6], CORPUS, 2)),
    # a match at the last corpus entry has no continuation: skipped, the search goes on (here to the shorter n-gram)
    (([9, 1, 2], [2, 4, 1, 2], 3, 2, None), ([4, 1, 2], CORPUS, 1)),
    (([9, 1, 2], [7, 1, 2], 3, 2, None), ([], NONE, 0)),
    # a match in front of a separator likewise; the later window with an id behind it is taken
    (([9, 1, 2], [1, 2, -1, 1, 2, 4], 3, 2, None), ([4], CORPUS, 2)),
    # the lower index wins among equal n
    (([9, 1, 2], [1, 2, 4, 4, 1, 2, 5, 5], 2, 2, None), ([4, 4], CORPUS, 2)),
    # len = 2, the empty corpus, K and the cut at max_positions
    (([5, 5], [], 3, 2, None), ([5], HISTORY, 1)),
    (([4, 5], [5, 6, 7, 8], 3, 16, None), ([6, 7, 8], CORPUS, 1)),
    (([4, 5], [5, 6, 7, 8], 1, 16, None), ([6], CORPUS, 1)),
    (([4, 5], [5, 6, 7, 8], 3, 16, 4), ([6, 7], CORPUS, 1)),
    (([4, 5], [5, 6, 7, 8], 3, 16, 3), ([6], CORPUS, 1)),
    (([4, 5], [5, 6, 7, 8], 3, 16, 2), ([], NONE, 0)),
    (([5], [5, 6, 7, 8], 3, 2, None), ([], NONE, 0)),
]


# ------------------------------------------------------------------------------------------ the rule
def test_the_two_formulations_agree_on_random_cases():
    rng = random.Random(11)
    n = hits = 0
    for L in (0, 1, 2, 3, 5, 9, 20):
        for C in (0, 1, 2, 3, 7, 30, 90):
            for _ in range(8):
                ids = [rng.randrange(4) for _ in range(L)]
                corpus = [(-1 if rng.random() < 0.12 else rng.randrange(4)) for _ in range(C)]
                for K in (1, 2, 3):
                    for ng in (1, 2, 5, 16):
                        for cap in (None, L, L + 1, L + 2):
                            got = oracle.lookup_corpus(ids, corpus, K, ng, cap)
                            assert got == oracle.lookup_corpus_brute(ids, corpus, K, ng, cap), (ids, corpus, K, ng, cap)
                            n += 1
                            hits += got[1] == CORPUS
    assert n > 4000 and hits > 300


def test_an_empty_corpus_is_the_rule_of_the_history_alone():
    rng = random.Random(12)
    for alphabet in (2, 4, 50):
        for L in list(range(0, 10)) + [17, 40]:
            for _ in range(5):
                ids = [rng.randrange(alphabet) for _ in range(L)]
                for K in (1, 2, 3):
                    for ng in (1, 2, 4):
                        for cap in (None, L, L + 1, L + 2, L + 7):
                            want = spec_oracle.lookup(ids, K, ng, cap)
                            for f in (oracle.lookup_corpus, oracle.lookup_corpus_brute):
                                drafts, src, n = f(ids, [], K, ng, cap)
                                assert drafts == want and (src == HISTORY) == bool(want) and src != CORPUS, (ids, K, ng, cap)


@pytest.mark.parametrize("case, want", KNOWN)
def test_known_answers(case, want):
    assert oracle.lookup_corpus(*case) == want
    assert oracle.lookup_corpus_brute(*case) == want


def test_accept_pattern_takes_the_drafts_of_the_corpus():
    T, K = 4, 3
    seq = [9, 9, 9, 1] + list(range(100, 130))
    corpus = [1] + list(range(100, 130))            # the whole continuation: every step behind the first accepts K + 1
    steps = oracle.steps_corpus(seq, T, K, 2, corpus, 12, 2048)
    assert [a for a, _, _ in steps] == [1, 4, 4, 4] and all(s == CORPUS for _, _, s in steps[1:])
    assert oracle.accept_pattern_corpus(seq, T, K, 2, corpus, 12, 2048) == [1, 4, 4, 4]
    assert oracle.accept_pattern_corpus(seq, T, K, 2, [], 6, 2048) == [1] * 6
    wrong = oracle.flatten([[t, 999] for t in range(100, 130)])      # every token is followed by a wrong one: a draft per step, none accepted
    steps = oracle.steps_corpus(seq, T, K, 2, wrong, 6, 2048)
    assert [a for a, _, _ in steps] == [1] * 6 and all((k, s) == (1, CORPUS) for _, k, s in steps[1:])


def test_flatten():
    assert oracle.flatten([[1, 2], [], [3]]) == [1, 2, -1, 3] == flatten_corpus([[1, 2], torch.tensor([], dtype=torch.int64), torch.tensor([3])], 10)
    assert flatten_corpus(None, 10) == [] and flatten_corpus([], 10) == [] and flatten_corpus([[]], 10) == []


# ------------------------------------------------------------------------------------------ the C ABI
def test_abi_is_additive():
    header = (Path(__file__).resolve().parents[1] / "include" / "dtk.h").read_text()
    lib = _lib.load_library()
    assert re.search(r"^#define DTK_ABI_VERSION 7\b", header, re.M) and lib.dtk_abi_version() == 7 == _lib.DTK_ABI_VERSION
    for name in NEW:
        decl = re.search(rf"^int\s+{name}\((.*?)\);", header, re.M | re.S)
        assert decl, f"{name} is not declared in dtk.h"
        assert name in _lib.SYMBOLS and name in _lib.CORPUS_SYMBOLS and getattr(lib, name).argtypes is not None
        assert len(_lib.SYMBOLS[name][1]) == decl.group(1).count(",") + 1, name
    assert re.search(r"#define\s+DTK_SPEC_CORPUS_MAX\s+%d\b" % _lib.DTK_SPEC_CORPUS_MAX, header) and _lib.DTK_SPEC_CORPUS_MAX == oracle.CORPUS_MAX
    for name, value in (("NONE", NONE), ("HISTORY", HISTORY), ("CORPUS", CORPUS)):
        assert re.search(r"#define\s+DTK_SPEC_FROM_%s\s+%d\b" % (name, value), header) and getattr(_lib, "DTK_SPEC_FROM_" + name) == value


# ------------------------------------------------------------------------------------------ generate(): checks
class CorpusDevice(SpecDevice):
    """SpecDevice with the corpus wrappers recorded"""

    def __init__(self, *a, fail_in_step=False, **kw):
        super().__init__(*a, **kw)
        self.corpus, self.fail_in_step = [], fail_in_step

    def _spec_set_corpus(self, flat):
        assert self.spec is None, "the corpus changes only outside a speculation"
        self.calls.append(("set_corpus", list(flat)))
        self.corpus = list(flat)

    def spec_corpus_len(self):
        return len(self.corpus)

    def spec_counters(self):
        assert self.spec is None
        self.calls.append(("spec_counters",))
        return (3, 2, 1)

    def spec_wait(self, logprobs=False):
        if self.fail_in_step:
            raise RuntimeError("the device went away")
        toks = self.spending.pop(0)
        return (toks, [0.0] * len(toks), [0.0] * len(toks)) if logprobs else toks

    def enable_logprobs(self):
        pass


def _call(extra=()):
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0, extra=list(extra))
    return ids, dict(input_ids=ids[None], pixel_values=px, max_new_tokens=8, **GEN)


def test_validation_errors_of_generate():
    ids, call = _call()
    dev = CorpusDevice(slots=5)
    with pytest.raises(ValueError, match="prompt_lookup_corpus without prompt_lookup_num_tokens"):
        dev.generate(prompt_lookup_corpus=[[5, 6]], **call)
    with pytest.raises(ValueError, match="prompt_lookup_corpus without prompt_lookup_num_tokens"):
        dev.generate(prompt_lookup_corpus=[[5, 6]], prompt_lookup_num_tokens=0, **call)
    for bad in ([[5, VOCAB]], [[-1, 5]], [[5, 6.0]], [[True]], [torch.tensor([VOCAB])], [torch.zeros(2, 2, dtype=torch.int64)], [5, 6],
                torch.tensor([5, 6])):
        with pytest.raises(ValueError, match="prompt_lookup_corpus"):
            dev.generate(prompt_lookup_corpus=bad, prompt_lookup_num_tokens=2, **call)
    half = [5] * (_lib.DTK_SPEC_CORPUS_MAX // 2)
    with pytest.raises(ValueError, match="prompt_lookup_corpus.*exceed %d" % _lib.DTK_SPEC_CORPUS_MAX):      # the separator is the entry too many
        dev.generate(prompt_lookup_corpus=[half, half], prompt_lookup_num_tokens=2, **call)
    assert dev.calls == []
    dev.generate(prompt_lookup_corpus=[half, half[:-1]], prompt_lookup_num_tokens=2, **call)
    sets = [c[1] for c in dev.calls if c[0] == "set_corpus"]
    assert len(sets) == 2 and len(sets[0]) == _lib.DTK_SPEC_CORPUS_MAX and sets[0][len(half)] == -1 and sets[1] == []


def test_a_fake_or_library_without_the_corpus_calls():
    ids, call = _call()
    bare = SpecDevice(slots=5)          # the speculative wrappers without the corpus ones: works with the argument off ...
    want = bare.generate(prompt_lookup_num_tokens=2, **call)
    with pytest.raises(_lib.DtkError, match="corpus"):      # ... and says what is missing with it on
        SpecDevice(slots=5).generate(prompt_lookup_num_tokens=2, prompt_lookup_corpus=[[5, 6]], **call)
    dev = CorpusDevice(slots=5)
    assert torch.equal(dev.generate(prompt_lookup_num_tokens=2, prompt_lookup_corpus=[[5, 6]], **call), want)
    for empty in (None, [], [[]], [[], torch.tensor([], dtype=torch.int64)]):      # nothing to set: the calls of a call without the argument
        plain = CorpusDevice(slots=5)
        assert torch.equal(plain.generate(prompt_lookup_num_tokens=2, prompt_lookup_corpus=empty, **call), want)
        assert plain.calls == bare.calls


def test_the_corpus_is_set_before_spec_begin_and_cleared_after_spec_end():
    ids, call = _call()
    dev = CorpusDevice(slots=5)
    out = dev.generate(prompt_lookup_num_tokens=2, prompt_lookup_corpus=[[5, 6], [], torch.tensor([7])], return_logprobs=True, **call)
    names = [c[0] for c in dev.calls]
    assert dev.calls[names.index("set_corpus")] == ("set_corpus", [5, 6, -1, 7])
    assert names.index("prefill") < names.index("set_corpus") == names.index("spec_begin") - 1
    assert names[-3:] == ["spec_end", "spec_counters", "set_corpus"] and dev.calls[-1] == ("set_corpus", []) and dev.spec_corpus_len() == 0
    assert isinstance(out, GenerateOutput) and out.draft_sources == (3, 2, 1) and sum(out.accepted_per_step) >= 8
    # a later call without the argument sees none, and reports no sources
    n = len(dev.calls)
    out = dev.generate(prompt_lookup_num_tokens=2, return_logprobs=True, **call)
    assert all(c[0] not in ("set_corpus", "spec_counters") for c in dev.calls[n:]) and out.draft_sources is None


def test_the_corpus_is_cleared_when_generate_raises():
    ids, call = _call()
    dev = CorpusDevice(slots=5, fail_in_step=True)
    with pytest.raises(RuntimeError, match="went away"):
        dev.generate(prompt_lookup_num_tokens=2, prompt_lookup_corpus=[[5, 6]], **call)
    assert dev.calls[-1] == ("set_corpus", []) and dev.spec_corpus_len() == 0 and dev.spec is None and not dev._single_busy.locked()

    class EndFails(CorpusDevice):
        def spec_end(self, keep_len):
            super().spec_end(keep_len)
            raise _lib.DtkError("dtk_spec_end failed")

    dev = EndFails(slots=5)
    with pytest.raises(_lib.DtkError, match="dtk_spec_end"):
        dev.generate(prompt_lookup_num_tokens=2, prompt_lookup_corpus=[[5, 6]], **call)
    assert dev.calls[-1] == ("set_corpus", []) and not dev._single_busy.locked()


# ------------------------------------------------------------------------------------------ the generator's corpus
class _Model(FakeModel):
    def __init__(self):
        super().__init__()
        self.seen = []

    def generate(self, **kw):
        self.seen.append(kw.get("prompt_lookup_corpus"))
        return super().generate(**{k: v for k, v in kw.items() if not k.startswith(("prompt_lookup", "max_matching"))})


def _generator(model, **kw):
    proc = fake_processor(512, 12)
    return DetikzifyGenerator(model, proc, sketch_image(1, 96), max_length=30, **kw)


def _program(gen, doc_ids):
    return [int(t) for t in doc_ids[int(gen.montecarlo.root_node.token_ids.numel()):]]


def test_generator_keeps_the_last_rollouts_newest_first():
    model = _Model()
    gen = _generator(model, prompt_lookup_num_tokens=3, prompt_lookup_rollouts=2)
    root = gen.montecarlo.root_node.token_ids
    programs = [_program(gen, gen.generate(root)) for _ in range(4)]
    assert all(programs) and len({tuple(p) for p in programs}) == 4
    assert model.seen == [None, [programs[0]], [programs[1], programs[0]], [programs[2], programs[1]]]      # R = 2 newest, newest first
    # explicit sequences come first, whether given to the generator or to the call; empty ones are dropped
    model = _Model()
    gen = _generator(model, prompt_lookup_num_tokens=3, prompt_lookup_rollouts=3, prompt_lookup_corpus=[[7, 8, 9], []])
    first = _program(gen, gen.generate(root))
    second = _program(gen, gen.generate(root))
    gen.generate(root, prompt_lookup_corpus=[torch.tensor([4, 5])])
    assert model.seen == [[[7, 8, 9]], [[7, 8, 9], first], [[4, 5], second, first]]
    # a rollout that continues a node keeps the whole program part behind the ROOT prompt
    gen.generate(torch.cat([root, torch.tensor([33, 34])]))
    assert list(gen._rollouts)[-1][:2] == [33, 34]


def test_generator_trims_the_oldest_rollouts_at_the_cap(monkeypatch):
    model = _Model()
    gen = _generator(model, prompt_lookup_num_tokens=2, prompt_lookup_rollouts=8, prompt_lookup_corpus=[[7, 8, 9]])
    root = gen.montecarlo.root_node.token_ids
    programs = [_program(gen, gen.generate(root)) for _ in range(5)]
    newest = programs[::-1]
    for cap in (3, 3 + 1 + len(newest[0]) - 1, 3 + 1 + len(newest[0]), 3 + 2 + len(newest[0]) + len(newest[1]), 10 ** 6):
        monkeypatch.setattr(_lib, "DTK_SPEC_CORPUS_MAX", cap)
        got = gen._lookup_corpus([[7, 8, 9]])
        assert got[0] == [7, 8, 9] and got[1:] == newest[:len(got) - 1]
        assert len(oracle.flatten(got)) <= cap
        if len(got) - 1 < len(newest):      # the next one would not have fitted
            assert len(oracle.flatten(got + [newest[len(got) - 1]])) > cap
    assert len(gen._lookup_corpus([[7, 8, 9]])) == 6


def test_generator_passes_nothing_when_off():
    root = None
    for kw in (dict(prompt_lookup_num_tokens=3), dict(prompt_lookup_num_tokens=3, prompt_lookup_rollouts=0), dict(prompt_lookup_rollouts=4),
               dict(prompt_lookup_num_tokens=0, prompt_lookup_rollouts=4), dict()):
        model = _Model()
        gen = _generator(model, **kw)
        root = gen.montecarlo.root_node.token_ids
        for _ in range(3):
            gen.generate(root)
        assert model.seen == [None] * 3 and not gen._rollouts, kw
    with pytest.raises(ValueError, match="prompt_lookup_rollouts"):
        _generator(_Model(), prompt_lookup_rollouts=-1)
    # the pipeline forwards the argument like every generation argument
    from detikzify_amd.infer.pipeline import DetikzifyPipeline
    model = _Model()
    pipe = DetikzifyPipeline(model, fake_processor(512, 12), metric="fast", prompt_lookup_num_tokens=2, prompt_lookup_rollouts=2, max_length=30)
    items = list(pipe.simulate(sketch_image(1, 96), expansions=4))
    assert len(items) == 4 and len(model.seen) >= 2 and model.seen[0] is None and all(1 <= len(s) <= 2 for s in model.seen[1:])
