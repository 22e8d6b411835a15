"""Classifier-free guidance, host side (no GPU): the additive C ABI, the argument checks of generate() — which run before any library
call — and the call sequence of a guided generate() on a scripted device: slot-0 settings, neutral slot 1, two prefills, the pair,
launches of [0, 1], and the pair dissolved again however the call ends."""
import math
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from detikzify_amd import _lib
from detikzify_amd.infer.batching import BatchEngine
from detikzify_amd.infer.generate import DetikzifyGenerator
from detikzify_amd.model.adapter_processing import AdapterProcessor
from detikzify_amd.model.modeling import _NEUTRAL_GENERATE_KWARGS, check_guidance_scale
from detikzify_amd.model.tokenizer import SyntheticTokenizer

from . import cfg_oracle
from .helpers import fake_processor, sketch_image
from .test_generate_loop import EOS, IMG, NIMG, VOCAB, ScriptedDevice, _prompt

NEW = ("dtk_set_guidance", "dtk_get_guidance", "dtk_op_cfg_mix", "dtk_bench_cfg")


class GuidedDevice(ScriptedDevice):
    """ScriptedDevice that records the wrapper calls generate() makes and plays the follower: in a step of a guided pair the
    unconditional slot reports (and appends) the conditional slot's token.  disagree_at = n: step n of the pair is left as the two
    slots' own tokens"""

    def __init__(self, slots=0, disagree_at=None, **kw):
        super().__init__(slots=slots, **kw)
        self.calls, self.pair, self.steps, self.disagree_at = [], None, 0, disagree_at

    def set_sampling(self, *a, **kw):
        self.calls.append(("set_sampling", kw.get("slot"), bool(a[0] if a else kw.get("do_sample", False))))
        super().set_sampling(*a, **kw)

    def prefill(self, input_ids, pixel_values=None, **kw):
        self.calls.append(("prefill", kw.get("slot"), [int(t) for t in input_ids.reshape(-1)],
                           None if pixel_values is None else float(pixel_values.float().sum())))
        super().prefill(input_ids, pixel_values, **kw)

    def set_guidance(self, scale, cond_slot, uncond_slot):
        assert not self.bpending, "set_guidance while a batched step is un-collected"
        g = check_guidance_scale(scale)
        self.calls.append(("set_guidance", scale, cond_slot, uncond_slot))
        self.pair = None if (uncond_slot is None or g == 1.0) else (cond_slot, uncond_slot, g)

    def decode_launch(self):
        self.calls.append(("decode_launch",))
        super().decode_launch()

    def decode_batch_launch(self, active_slots):
        slots = list(active_slots)
        self.calls.append(("decode_batch_launch", slots))
        super().decode_batch_launch(slots)
        if self.pair and self.pair[0] in slots and self.steps != self.disagree_at:
            c, u, _ = self.pair
            self.bpending[-1][u] = self.bpending[-1][c]
            self.ctx[u][-1] = self.bpending[-1][c]
        elif self.pair:
            c, u, _ = self.pair
            self.bpending[-1][u] = self.bpending[-1][c] + 1       # (the toy's two slots could agree by chance)
        self.steps += 1

    def synchronize(self):
        self.calls.append(("synchronize",))


def test_abi_is_additive():
    header = (Path(__file__).resolve().parents[1] / "include" / "dtk.h").read_text()
    lib = _lib.load_library()
    assert re.search(r"^#define DTK_ABI_VERSION 7\b", header, re.M) and lib.dtk_abi_version() == 7 == _lib.DTK_ABI_VERSION
    for name in NEW:
        assert re.search(r"^int\s+%s\(" % name, header, re.M), f"{name} is not declared in dtk.h"
        assert name in _lib.SYMBOLS and getattr(lib, name).argtypes is not None
    assert "guidance_scale" not in _NEUTRAL_GENERATE_KWARGS and "negative_prompt_ids" not in _NEUTRAL_GENERATE_KWARGS
    assert _NEUTRAL_GENERATE_KWARGS["negative_prompt_attention_mask"] == (None,)


def test_oracle_replay_is_the_formula():
    rng = np.random.default_rng(0)
    zc, zu = rng.standard_normal(1000).astype(np.float32) * 8, rng.standard_normal(1000).astype(np.float32) * 8
    for g in (0.0, 0.5, 1.5, 3.0, 7.5):
        want, Lc, Lu = cfg_oracle.mix64(zc, zu, g)
        got = cfg_oracle.out32(zc, zu, g, Lc, Lu)
        assert got.dtype == np.float32 and np.abs(got - want).max() < 1e-4 * max(1.0, g)
    same = cfg_oracle.out32(zc, zc, 3.0, 1.25, 1.25)
    assert same.tobytes() == (zc - np.float32(1.25)).tobytes()
    assert cfg_oracle.out32(zc, zu, 0.0, 2.0, 3.0).tobytes() == (zu - np.float32(3.0)).tobytes()


GEN = dict(bad_words_ids=[[IMG]], begin_suppress_tokens=[EOS], do_sample=True, seed=7)


@pytest.mark.parametrize("g", [None, 1.0, 1])
def test_neutral_values_make_the_calls_of_a_plain_generate(g):
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0)
    plain, dev = GuidedDevice(slots=5), GuidedDevice(slots=5)
    want = plain.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=12, **GEN)
    got = dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=12, guidance_scale=g, negative_pixel_values=px * 0, **GEN)
    assert torch.equal(got, want) and dev.calls == plain.calls
    assert all(c[0] in ("set_sampling", "prefill", "decode_launch") and (len(c) < 2 or c[1] is None) for c in dev.calls)


@pytest.mark.parametrize("g", [-0.1, 100.5, float("nan"), float("inf"), "2", True])
def test_bad_values_raise_before_any_call(g):
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0)
    dev = GuidedDevice(slots=5)
    with pytest.raises(ValueError, match="guidance_scale"):
        dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=4, guidance_scale=g, negative_pixel_values=px * 0, **GEN)
    assert dev.calls == []
    dev.generation_config.guidance_scale = g
    with pytest.raises(ValueError, match="guidance_scale"):
        dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=4, negative_pixel_values=px * 0, **GEN)
    assert dev.calls == []


def test_guidance_needs_a_negative_slots_and_no_engine():
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0)
    dev = GuidedDevice(slots=5)
    with pytest.raises(ValueError, match="negative_pixel_values"):
        dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=4, guidance_scale=2.0, **GEN)
    for slots in (0, 1):
        small = GuidedDevice(slots=slots)
        with pytest.raises(ValueError, match="batch_slots"):
            small.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=4, guidance_scale=2.0, negative_pixel_values=px * 0, **GEN)
        assert small.calls == []
    eng = BatchEngine(dev, max_batch=4)
    try:
        seen = []
        eng.sequence = lambda *a, **k: seen.append(a) or (_ for _ in ()).throw(AssertionError("the engine saw a sequence"))
        with pytest.raises(NotImplementedError, match="guidance_scale: not in the batch engines yet"):
            dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=4, guidance_scale=2.0, negative_pixel_values=px * 0, **GEN)
        assert seen == []
    finally:
        del eng.sequence
        eng.close()
    assert dev.calls == []
    # the text-only case: no image on either side and no negative text
    with pytest.raises(ValueError, match="negative_adapter_input_ids"):
        dev.generate(input_ids=ids[None], max_new_tokens=4, guidance_scale=2.0, negative_prompt_ids=ids[None], **GEN)


def _guided(dev, ids, px, px2, **kw):
    return dev.generate(input_ids=ids[None], pixel_values=px, guidance_scale=2.5, negative_pixel_values=px2, **{**GEN, **kw})


def test_call_order_of_a_guided_generate():
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0, extra=[40, 41])
    _, px2 = _prompt(proc, 3)
    dev = GuidedDevice(slots=5)
    out = _guided(dev, ids, px, px2, max_new_tokens=6, suppress_tokens=[EOS], eos_token_id=-1)
    T = ids.numel()
    assert out.shape == (1, T + 6)
    names = [c[0] for c in dev.calls]
    # slot-0 settings, neutral slot 1, the two prefills, the pair, then only launches of [0, 1] until the teardown
    assert dev.calls[0] == ("set_sampling", 0, True) and dev.calls[1] == ("set_sampling", 1, False)
    assert dev.calls[2][:3] == ("prefill", 0, ids.tolist()) and dev.calls[3][:3] == ("prefill", 1, ids.tolist())      # negative ids default to the prompt's
    assert dev.calls[2][3] == float(px.float().sum()) and dev.calls[3][3] == float(px2.float().sum())
    assert dev.calls[4] == ("set_guidance", 2.5, 0, 1)
    launches = [c for c in dev.calls if c[0] == "decode_batch_launch"]
    assert len(launches) == 6 and all(c == ("decode_batch_launch", [0, 1]) for c in launches)
    assert "decode_launch" not in names
    assert dev.calls[-1] == ("set_guidance", None, 0, None) and dev.pair is None and not dev.bpending
    assert names.index("synchronize") > max(i for i, n in enumerate(names) if n == "decode_batch_launch")
    assert dev.samp[1] == dict(do_sample=False, seed=0, bad_ids=(), begin_suppress_ids=(), always_suppress_ids=())
    assert dev.samp[0]["bad_ids"] == (IMG,) and dev.samp[0]["seed"] == 7
    # the two slots hold the same continuation behind their own prompts
    assert dev.ctx[0][T:] == out[0, T:].tolist() == dev.ctx[1][T:]
    # a negative prompt of its own, longer than the prompt: max_length is clamped by it
    neg = torch.cat([ids, torch.tensor([50, 51, 52, 53])])
    dev2 = GuidedDevice(slots=5, max_positions=T + 10)
    out2 = dev2.generate(input_ids=ids[None], pixel_values=px, guidance_scale=2.5, negative_prompt_ids=neg[None], suppress_tokens=[EOS],
                         eos_token_id=-1, max_length=10 ** 6, **GEN)
    assert dev2.calls[3][:3] == ("prefill", 1, neg.tolist()) and out2.shape == (1, T + 6)
    assert len(dev2.ctx[1]) == T + 10


def _raising_streamer(n):
    class S:
        seen = 0

        def put(self, value):
            if value.numel() == 1:
                self.seen += 1
                if self.seen == n:
                    raise RuntimeError("consumer gone")

        def end(self):
            pass
    return S()


@pytest.mark.parametrize("how", ["budget", "eos", "criterion", "streamer"])
def test_the_pair_is_dissolved_however_the_call_ends(how):
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0)
    _, px2 = _prompt(proc, 3)
    dev = GuidedDevice(slots=5)
    if how == "budget":
        _guided(dev, ids, px, px2, max_new_tokens=5, suppress_tokens=[EOS], eos_token_id=-1)
    elif how == "eos":
        out = _guided(dev, ids, px, px2, max_new_tokens=120)
        assert out[0, -1] == EOS
    elif how == "criterion":
        out = _guided(dev, ids, px, px2, max_new_tokens=30, suppress_tokens=[EOS], eos_token_id=-1,
                      stopping_criteria=[lambda i, s: i.shape[1] >= ids.numel() + 3])
        assert out.shape[1] == ids.numel() + 3
    else:
        with pytest.raises(RuntimeError, match="consumer gone"):
            _guided(dev, ids, px, px2, max_new_tokens=30, suppress_tokens=[EOS], eos_token_id=-1, streamer=_raising_streamer(3))
    assert dev.calls[-1] == ("set_guidance", None, 0, None) and dev.pair is None
    assert not dev.bpending                                         # the step left in flight was collected first
    # and the model is free again: a plain call makes plain calls
    n = len(dev.calls)
    dev.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=3, **GEN)
    assert all(c[0] in ("set_sampling", "prefill", "decode_launch") for c in dev.calls[n:])


def test_a_step_whose_two_tokens_disagree_raises():
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0)
    _, px2 = _prompt(proc, 3)
    dev = GuidedDevice(slots=5, disagree_at=2)
    with pytest.raises(_lib.DtkError, match="guided pair"):
        _guided(dev, ids, px, px2, max_new_tokens=10, suppress_tokens=[EOS], eos_token_id=-1)
    assert dev.calls[-1] == ("set_guidance", None, 0, None) and not dev.bpending


def test_generation_config_is_honoured():
    proc = fake_processor(VOCAB, NIMG)
    ids, px = _prompt(proc, 0)
    _, px2 = _prompt(proc, 3)
    dev = GuidedDevice(slots=5)
    dev.generation_config.guidance_scale = 3.0
    dev.generate(input_ids=ids[None], pixel_values=px, negative_pixel_values=px2, max_new_tokens=4, suppress_tokens=[EOS], eos_token_id=-1, **GEN)
    assert ("set_guidance", 3.0, 0, 1) in dev.calls
    assert dev.calls[2][:3] == ("prefill", 0, ids.tolist()) and dev.calls[3][:3] == ("prefill", 1, ids.tolist())
    # the argument wins over the configuration
    n = len(dev.calls)
    dev.generate(input_ids=ids[None], pixel_values=px, negative_pixel_values=px2, guidance_scale=1.0, max_new_tokens=4, **GEN)
    assert all(c[0] != "set_guidance" for c in dev.calls[n:])
    assert check_guidance_scale(None) == 1.0 and check_guidance_scale(0) == 0.0 and check_guidance_scale(100) == 100.0
    assert math.isclose(check_guidance_scale(np.float64(1.5)), 1.5)


class _RecordingModel:
    """the attribute surface DetikzifyGenerator.generate touches; generate() records its arguments"""

    def __init__(self):
        cfg = SimpleNamespace(image_token_id=IMG, eos_token_id=EOS)
        cfg.text_config = cfg
        self.config, self.device, self.seen = cfg, torch.device("cpu"), []
        self.generation_config = SimpleNamespace(to_dict=lambda: {"max_length": 64})

    def generate(self, input_ids=None, streamer=None, **kw):
        self.seen.append(kw)
        if streamer is not None:
            streamer.end()
        return input_ids


def test_generator_turns_negative_image_and_text_into_tensors():
    inner = fake_processor(VOCAB, NIMG)
    image, other = sketch_image(0, 96), sketch_image(4, 96)
    # image prompt: the negative image through the same processor; the default is a white canvas of the processor's size
    model = _RecordingModel()
    gen = DetikzifyGenerator(model, inner, image, guidance_scale=2.0, negative_image=other)
    gen.generate(gen.montecarlo.root_node.token_ids)
    kw = model.seen[-1]
    assert kw["guidance_scale"] == 2.0 and "negative_image" not in kw and "negative_text" not in kw
    assert torch.equal(kw["negative_pixel_values"], inner(images=other, return_tensors="pt").pixel_values)
    assert not torch.equal(kw["negative_pixel_values"], kw["pixel_values"])
    gen = DetikzifyGenerator(model, inner, image)
    gen.generate(gen.montecarlo.root_node.token_ids, guidance_scale=1.5)
    white = Image.new("RGB", (84, 84), color="white")
    assert torch.equal(model.seen[-1]["negative_pixel_values"], inner(images=white, return_tensors="pt").pixel_values)
    # off: nothing of it reaches the model
    gen.generate(gen.montecarlo.root_node.token_ids, negative_image=other)
    assert not any(k.startswith("negative") for k in model.seen[-1]) and "guidance_scale" not in model.seen[-1]
    gen.generate(gen.montecarlo.root_node.token_ids, guidance_scale=1.0, negative_image=other)
    assert not any(k.startswith("negative") for k in model.seen[-1])
    with pytest.raises(ValueError, match="guidance_scale"):
        gen.generate(gen.montecarlo.root_node.token_ids, guidance_scale=-1.0)
    with pytest.raises(ValueError, match="adapter"):
        gen.generate(gen.montecarlo.root_node.token_ids, guidance_scale=2.0, negative_text="a cat")
    # with the adapter's processor the negative text goes through the adapter's tokenizer; a text-only prompt needs one
    tok = SyntheticTokenizer(300, bos_token_id=1, eos_token_id=2, pad_token_id=0, model_max_length=512)
    proc = AdapterProcessor(inner, tok)
    gen = DetikzifyGenerator(model, proc, None, text="a red circle", guidance_scale=2.0, negative_text="a blue square")
    gen.generate(gen.montecarlo.root_node.token_ids)
    kw = model.seen[-1]
    assert torch.equal(kw["negative_adapter_input_ids"], proc(text="a blue square", return_tensors="pt")["adapter_input_ids"])
    assert "negative_pixel_values" not in kw and not torch.equal(kw["negative_adapter_input_ids"], kw["adapter_input_ids"])
    gen = DetikzifyGenerator(model, proc, None, text="a red circle", guidance_scale=2.0)
    with pytest.raises(ValueError, match="negative_text"):
        gen.generate(gen.montecarlo.root_node.token_ids)
    gen = DetikzifyGenerator(model, proc, image, text="a red circle", guidance_scale=2.0, negative_text="a blue square")
    gen.generate(gen.montecarlo.root_node.token_ids)
    kw = model.seen[-1]
    assert "negative_pixel_values" in kw and "negative_adapter_input_ids" in kw
