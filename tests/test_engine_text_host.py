"""Text-conditioned sequences (the TikZero adapter) in the batch engine's slots, on the CPU: the shipped native run loop
(dtk_engine_submit_text, dtk_engine_set_prefill_text_op) and the Python-driven BatchEngine over the scripted device of
tests/test_generate_loop.py, extended by a text prefill.  The scripted device keys a text-conditioned slot by the pair key
dtk_text_image_key(image key, text key) exactly as dtk_prefill_slot_text does, and its toy LM hashes that key: a sequence that got
another (image, text)'s prefix decodes other tokens, and every prefix-reusing prefill asserts that the slot really holds it.
What this pins without a GPU:

  * a text join calls the text prefill with its ids, its text, its image key and the prefix-reuse flags; text-only prompts use
    the dummy image's key;
  * the prefix cache is keyed by (image, text, prefix length): two texts on one image encode twice, the same text forks;
  * image-only and text joins of the same image never share a slot prefix nor resume into each other; resume in place happens
    only under the same (image, text);
  * a text join on an ops engine without the text op fails alone; the stale-source guard encodes a prefix again;
  * generate(adapter_input_ids=...) with an engine, and a fixed-seed simulate_parallel(text=...), give the same tokens under both
    engines as alone.
"""
import ctypes as C
import threading
from types import SimpleNamespace

import pytest
import torch

from detikzify_amd import _lib
from detikzify_amd.infer import DetikzifyPipeline, SyntheticTikzDocument
from detikzify_amd.infer.batching import BatchEngine, simulate_parallel, simulate_parallel_images
from detikzify_amd.infer.engine import NativeBatchEngine
from detikzify_amd.model import AdapterProcessor
from detikzify_amd.model.modeling import DUMMY_IMAGE_KEY, text_image_key, text_key
from detikzify_amd.model.tokenizer import SyntheticTokenizer

from .helpers import fake_processor, sketch_image
from .test_generate_loop import EOS, IMG, NIMG, VOCAB, ScriptedDevice, _Lib, _prompt

KW = dict(bad_words_ids=[[IMG]], begin_suppress_tokens=[EOS], do_sample=True, max_length=NIMG + 50)


class _TextLib(_Lib):
    def dtk_adapter_destroy(self, ctx):         # as the C side: every slot's cached ids are gone
        self.dev.ctx.clear()
        self.dev.img.clear()
        return 0


class TextDevice(ScriptedDevice):
    """ScriptedDevice with the adapter's text prefill: a text-conditioned slot is stored under the pair key"""

    def __init__(self, slots=0, adapter=True, **kw):
        super().__init__(slots=slots, **kw)
        self.lib = _TextLib(self)
        if adapter:
            self.adapter = self.embedding_model = self.adapter_config = SimpleNamespace()
        self.text_calls = []        # (slot, ids, text ids, image key, reuse) of every text prefill

    def prefill(self, input_ids, pixel_values=None, return_logits=False, reuse=None, slot=None, adapter_input_ids=None):
        if adapter_input_ids is None:
            return super().prefill(input_ids, pixel_values, return_logits, reuse, slot)
        assert self.has_adapter() and not self.bpending
        s = self.SINGLE if slot is None else slot
        ids = [int(t) for t in input_ids.reshape(-1)]
        tids = [int(t) for t in torch.as_tensor(adapter_input_ids).reshape(-1)]
        ikey = self.image_key(pixel_values) if pixel_values is not None else DUMMY_IMAGE_KEY
        key = text_image_key(ikey, text_key(torch.tensor(tids)))
        self.text_calls.append((s, list(ids), tids, ikey, bool(reuse)))
        if reuse:
            n = next((i for i, t in enumerate(ids) if t != IMG), len(ids))
            assert self.img.get(s) == key and self.ctx[s][:n] == ids[:n], "prefix reuse without the (image, text) prefix in the slot"
            self.tail_prefills += 1
        self.pending.clear()
        self.ctx[s], self.img[s], self.gen0[s] = ids, key, len(ids)
        self.prefills += 1


def _text(seed, n=9):
    return torch.randint(3, 300, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)


def _alone(jobs):
    dev = TextDevice()
    return [dev.generate(input_ids=i[None], pixel_values=p, seed=s, adapter_input_ids=t, **KW) if t is not None else
            dev.generate(input_ids=i[None], pixel_values=p, seed=s, **KW) for i, p, t, s in jobs]


def _run(dev, jobs, threads=4, owners=False):
    got, errs = [None] * len(jobs), []

    def worker(k):
        try:
            for j in range(k, len(jobs), threads):
                i, p, t, s = jobs[j]
                extra = {"adapter_input_ids": t} if t is not None else {}
                got[j] = dev.generate(input_ids=i[None], pixel_values=p, seed=s, sequence_owner=j if owners else None, **extra, **KW)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    ths = [threading.Thread(target=worker, args=(k,)) for k in range(threads)]
    [t.start() for t in ths]
    [t.join(timeout=90) for t in ths]
    assert not any(t.is_alive() for t in ths) and not errs, errs[:1]
    return got


def test_pair_key_is_the_libraries():
    lib = _lib.load_library()
    assert text_image_key(5, 7) == lib.dtk_text_image_key(5, 7) != 0
    assert text_image_key(5, 7) != text_image_key(5, 8) and text_image_key(0, 7) == 0 == text_image_key(5, 0)


@pytest.mark.parametrize("make", [NativeBatchEngine, BatchEngine])
def test_text_join_prefills_with_its_text_image_key_and_flags(make):
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0, extra=[40, 41])
    tids = _text(1)
    dev = TextDevice(slots=5)
    eng = make(dev, max_batch=4)
    out = dev.generate(input_ids=ids[None], pixel_values=px, seed=3, adapter_input_ids=tids[None], **KW)
    st = eng.stats()
    eng.close()
    assert torch.equal(out, _alone([(ids, px, tids, 3)])[0])
    ikey = dev.image_key(px)
    prefix_slot = eng.prefix_slot
    # the prefix encode into the prefix-cache slot (ids[0, NIMG), no reuse), then the tail after the fork (reuse); both with the text
    assert [(c[0], c[1], c[2], c[3], c[4]) for c in dev.text_calls] == [
        (prefix_slot, ids[:NIMG].tolist(), tids.tolist(), ikey, False), (0, ids.tolist(), tids.tolist(), ikey, True)]
    assert dev.prefills == 2 and dev.forks == 1 and st["prefix_encodes"] == 1
    # text only: the dummy image's key, no pixels
    dev2 = TextDevice(slots=5)
    eng2 = make(dev2, max_batch=4, share_prefix=False)
    ids2 = torch.tensor([IMG] * NIMG + [40], dtype=torch.int64)
    out2 = dev2.generate(input_ids=ids2[None], pixel_values=None, seed=4, adapter_input_ids=tids, **KW)
    eng2.close()
    assert torch.equal(out2, _alone([(ids2, None, tids, 4)])[0])
    assert dev2.text_calls == [(0, ids2.tolist(), tids.tolist(), DUMMY_IMAGE_KEY, False)]


@pytest.mark.parametrize("make", [NativeBatchEngine, BatchEngine])
def test_prefix_cache_is_keyed_by_image_and_text(make):
    """two texts on one image: two prefix encodes; the same text again: forks.  Image-only and text prompts of the same image
    never share a prefix: three keys, three encodes, and every sequence decodes exactly as alone"""
    proc = fake_processor(VOCAB, NIMG)
    ta, tb = _text(10), _text(11)
    jobs = []
    for k in range(12):
        ids, px = _prompt(proc, 0, extra=[50 + k])
        jobs.append((ids, px, (ta, tb, None)[k % 3], 200 + k))
    dev = TextDevice(slots=7)            # three prefix-cache slots: one per (image, text) key, no eviction
    eng = make(dev, max_batch=4)
    got = _run(dev, jobs)
    st = eng.stats()
    eng.close()
    for a, g in zip(_alone(jobs), got):
        assert torch.equal(a, g)
    assert st["prefix_encodes"] == 3 and st["resumed_in_place"] == 0
    keys = set(eng.prefix_cache)
    ikey = dev.image_key(jobs[0][1])
    assert keys == {(ikey, text_key(ta), NIMG), (ikey, text_key(tb), NIMG), (ikey, 0, NIMG)}
    encodes = [c for c in dev.text_calls if c[0] in eng.prefix_slots]
    assert sorted(tuple(c[2]) for c in encodes) == sorted([tuple(ta.tolist()), tuple(tb.tolist())])


@pytest.mark.parametrize("make", [NativeBatchEngine, BatchEngine])
def test_resume_in_place_only_under_the_same_image_and_text(make):
    """a tree comes back to its own rollout: under the same text it resumes in the slot; the same ids under another text, or under
    no text, must prefill (the slot's cache is another (image, text)'s)"""
    proc = fake_processor(VOCAB, NIMG)
    ta, tb = _text(20), _text(21)
    ids, px = _prompt(proc, 1, extra=[61])
    first = _alone([(ids, px, ta, 300)])[0][0]
    back = first[: NIMG + 1 + max(1, (first.numel() - NIMG - 1) // 2)]
    for second_text, resumes in ((ta, 1), (tb, 0), (None, 0)):
        dev = TextDevice(slots=5)
        eng = make(dev, max_batch=4)
        a = dev.generate(input_ids=ids[None], pixel_values=px, seed=300, sequence_owner=0, adapter_input_ids=ta, **KW)
        extra = {"adapter_input_ids": second_text} if second_text is not None else {}
        b = dev.generate(input_ids=back[None], pixel_values=px, seed=301, sequence_owner=0, **extra, **KW)
        st = eng.stats()
        eng.close()
        assert torch.equal(a[0], first)
        assert torch.equal(b, _alone([(back, px, second_text, 301)])[0]), second_text
        assert st["resumed_in_place"] == dev.resumes == resumes, (second_text, st)


def test_text_join_without_text_op_fails_alone():
    """an ops engine whose device has no text prefill refuses the text join in submit (DTK_ERR_STATE, error_out says why); the
    engine goes on with image-only sequences"""
    proc = fake_processor(VOCAB, NIMG)
    dev = TextDevice(slots=4, adapter=False)
    eng = NativeBatchEngine(dev, max_batch=3)
    ids, px = _prompt(proc, 2)
    with pytest.raises(_lib.DtkError, match="no text prefill"):
        with eng.sequence(ids, px, {}, max_new_tokens=4, text_ids=_text(1)):
            pass
    assert sorted(eng.free) == [0, 1, 2]
    out = dev.generate(input_ids=ids[None], pixel_values=px, seed=9, **KW)
    assert torch.equal(out, TextDevice().generate(input_ids=ids[None], pixel_values=px, seed=9, **KW))
    # the raw C ABI: the same refusal
    j = _lib.DtkJoin()
    t = _text(2)
    j.slot, j.n_ids, j.ids, j.prefix_src, j.max_new_tokens = 0, ids.numel(), ids.data_ptr(), -1, 4
    ticket = C.c_uint64(0)
    rc = eng.lib.dtk_engine_submit_text(eng._h, C.byref(j), C.cast(t.data_ptr(), C.POINTER(C.c_int64)), t.numel(), 5, C.byref(ticket))
    assert rc == -3 and b"dtk_engine_set_prefill_text_op" in j.error_out
    assert eng.lib.dtk_engine_submit_text(eng._h, C.byref(j), None, 0, 5, C.byref(ticket)) == -1
    eng.close()


@pytest.mark.parametrize("text", [True, False])
def test_stale_prefix_cache_slot_is_encoded_again(text):
    """the bookkeeping says a prefix-cache slot holds (image, text) but the slot was overwritten behind its back: the native loop
    checks the source before the whole fork and encodes the prefix again instead of forking stale rows"""
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 3, extra=[70])
    t = _text(30) if text else None
    dev = TextDevice(slots=5)
    eng = NativeBatchEngine(dev, max_batch=4, resume_in_place=False)
    jobs = [(ids, px, t, 400), (ids, px, t, 401)]
    want = _alone(jobs)
    assert torch.equal(_run(dev, jobs[:1], threads=1)[0], want[0])
    src = eng.prefix_slot
    assert src in dev.ctx and eng.prefix_cache
    dev.ctx[src] = [IMG] * (NIMG - 1) + [99]        # (what a failed join can leave behind)
    before = dev.prefills
    assert torch.equal(_run(dev, jobs[1:], threads=1)[0], want[1])
    eng.close()
    assert dev.prefills == before + 2 and dev.ctx[src] == ids[:NIMG].tolist()      # encoded again + the tail


@pytest.mark.parametrize("make", [NativeBatchEngine, BatchEngine])
def test_generate_with_text_decodes_in_a_slot_among_others(make):
    """generate(adapter_input_ids=...) with an engine: texts, the same texts on other images, text only (dummy image) and
    image-only prompts in one batch — every sequence the tokens it gets alone"""
    proc = fake_processor(VOCAB, NIMG)
    texts = [_text(40), _text(41), None]
    jobs = []
    for k in range(15):
        ids, px = _prompt(proc, k % 2, extra=[80 + k][: k % 2])
        if k % 5 == 4:
            ids, px = torch.tensor([IMG] * NIMG + [90 + k], dtype=torch.int64), None
        t = texts[k % 3] if px is not None else texts[k % 2]
        jobs.append((ids, px, t, 500 + k))
    dev = TextDevice(slots=10)
    eng = make(dev, max_batch=8)
    got = _run(dev, jobs, threads=6, owners=True)
    eng.close()
    for a, g in zip(_alone(jobs), got):
        assert torch.equal(a, g)


def test_adapter_unload_makes_the_engines_forget_their_prefixes():
    """unload_cross_attn_adapter() clears every slot's cached ids on the C side: both engines forget which slot holds what
    (no fork from a slot that holds nothing any more); while a sequence decodes in a slot it is refused"""
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 4, extra=[33])
    t = _text(50)
    for make in (NativeBatchEngine, BatchEngine):
        dev = TextDevice(slots=6)
        eng = make(dev, max_batch=4)
        dev.generate(input_ids=ids[None], pixel_values=px, seed=1, adapter_input_ids=t, **KW)
        dev.generate(input_ids=ids[None], pixel_values=px, seed=2, **KW)
        assert len(eng.prefix_cache) == 2
        with eng.sequence(ids, px, dict(do_sample=True, seed=3), max_new_tokens=3):
            with pytest.raises(_lib.DtkError, match="while sequences decode"):
                dev.unload_cross_attn_adapter()
        dev.unload_cross_attn_adapter()
        assert not dev.has_adapter() and not dev.ctx
        out = dev.generate(input_ids=ids[None], pixel_values=px, seed=2, **KW)       # scripted kv_fork asserts a real source
        eng.close()
        assert torch.equal(out, TextDevice().generate(input_ids=ids[None], pixel_values=px, seed=2, **KW))
        assert list(eng.prefix_cache) == [(dev.image_key(px), 0, NIMG)]


def _adapter_processor():
    return AdapterProcessor(fake_processor(VOCAB, NIMG), SyntheticTokenizer(300, bos_token_id=1, eos_token_id=2, pad_token_id=0,
                                                                            model_max_length=64))


def test_both_engines_run_the_same_text_conditioned_search(monkeypatch):
    """simulate_parallel(text=...) and simulate_parallel_images(texts=...) with a fixed seed under DTK_ENGINE=python and the
    native loop: the same rollouts and scores; the text changes the search"""
    proc = _adapter_processor()
    image = sketch_image(9, 96)

    def run(kind, text, images=None, texts=None):
        monkeypatch.setenv("DTK_ENGINE", kind)
        dev = TextDevice(slots=14)
        pipe = DetikzifyPipeline(dev, proc, metric="fast", document_class=SyntheticTikzDocument, max_length=NIMG + 40, compile_timeout=None)
        if images is None:
            res = sorted((doc.code, score) for score, doc in simulate_parallel(pipe, image, trees=8, expansions_per_tree=3, text=text))
        else:
            res = sorted((i, doc.code, score) for i, score, doc in simulate_parallel_images(pipe, images, 3, 2, texts=texts))
        return res, dev.last_batch_stats
    py, st_py = run("python", "a red circle")
    nat, st_nat = run("native", "a red circle")
    assert len(py) == 24 and py == nat
    assert st_nat["joins"] == st_py["joins"] and st_nat["resumed_in_place"] == st_py["resumed_in_place"]
    assert run("native", None)[0] != nat
    images, texts = [image, None, image], ["a red circle", "a blue square", None]
    py, _ = run("python", None, images, texts)
    nat, st = run("native", None, images, texts)
    assert len(py) == 18 and py == nat and {i for i, _, _ in nat} == {0, 1, 2}
    # the pipeline routes simulate(text=..., trees=N) there
    monkeypatch.setenv("DTK_ENGINE", "native")
    dev = TextDevice(slots=6)
    pipe = DetikzifyPipeline(dev, proc, metric="fast", document_class=SyntheticTikzDocument, max_length=NIMG + 40, compile_timeout=None)
    got = list(pipe.simulate(text="a blue square", trees=4, expansions=2))
    assert len(got) == 8 and dev.last_batch_stats["engine"] == "native"
