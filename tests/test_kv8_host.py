"""The host side of kv_format "mxfp8" (no GPU): the C ABI's additions, load()'s refusals (raised before the library is touched), the
kv8 oracle against the plain one, and the teeth of the op-test inputs after quantisation — every input tests/test_gpu_kv8_attn.py
feeds to dtk_op_attn_decode_b8 is built here too: the spotlights must keep >= 0.99 of their mass on the de-quantised rows, and the
float64 reference on the de-quantised rows must be >= 1e-2 rel-L2 (five times the op bar) from the bf16 one, so a kernel that reads
the wrong copy of a region cannot pass."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from oracle.llama import LlamaOracle, mx_fake_quant, mx_quantise
from oracle.synth import make_weights
from tests import attn_decode_cases as ac
from tests import kv8_cases as kc
from tests.helpers import TINY_CFG
from tests.kv8_oracle import Kv8LlamaOracle

ROOT = Path(__file__).resolve().parent.parent
NEW = ("dtk_kv8_info", "dtk_read_kv8", "dtk_op_attn_decode_b8")
HOST_MODES = ("L", "mid", "pos")          # from = 0 is "L" of a slot that shares nothing


def test_header_declares_the_functions_and_symbols_list_them():
    header = (ROOT / "include" / "dtk.h").read_text()
    for name in NEW:
        assert re.search(rf"^int\s+{name}\(", header, re.M), name
        assert name in _lib.SYMBOLS, name
    assert len(_lib.SYMBOLS["dtk_op_attn_decode_b8"][1]) == 23
    assert len(_lib.SYMBOLS["dtk_read_kv8"][1]) == 9
    assert re.search(r"#define\s+DTK_ABI_VERSION\s+7\b", header) and _lib.DTK_ABI_VERSION == 7
    assert "[4] = key/value row format" in header


def test_load_refusals_come_before_the_library(monkeypatch):
    from detikzify_amd import model as M

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load_library", no_library)
    with pytest.raises(ValueError, match="kv_format"):
        M.load("detikzify-tiny", synthetic=1, batch_slots=4, kv_format="fp8")
    with pytest.raises(ValueError, match="kv_format"):
        M.load("detikzify-tiny", synthetic=1, kv_format="int8")
    with pytest.raises(NotImplementedError, match="kv_format='mxfp8'"):
        M.load("detikzify-tiny", synthetic=1, kv_format="mxfp8")
    with pytest.raises(NotImplementedError, match="kv_format='mxfp8'"):
        M.load("detikzify-ds-7b", synthetic=1, batch_slots=0, kv_format="mxfp8", weight_format="mxfp4")
    with pytest.raises(NotImplementedError):      # tl-1.1b and MXFP4 have no slots at all
        M.load("detikzify-tl-1.1b", synthetic=1, batch_slots=4, kv_format="mxfp8")
    with pytest.raises(NotImplementedError):
        M.load("detikzify-ds-7b", synthetic=1, batch_slots=4, kv_format="mxfp8", weight_format="mxfp4")
    from detikzify_amd.model.config import DetikzifyConfig
    assert DetikzifyConfig().kv_format == "bf16"


def _llama_pair():
    cfg = dict(TINY_CFG)
    w = make_weights(cfg, 99)
    return cfg, w


def test_oracle_with_the_boundary_at_or_beyond_the_length_is_the_plain_oracle():
    cfg, w = _llama_pair()
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(3, cfg["vocab"], (12,), generator=g)
    plain, kv8 = LlamaOracle(cfg, w), Kv8LlamaOracle(cfg, w)
    x = plain.embed(ids)
    for frm in (12, 13, 1 << 30):
        plain.reset(); kv8.reset()
        kv8.kv_from = frm
        a, b = plain.forward(x), kv8.forward(x)
        assert torch.equal(a, b), frm
        for i in range(plain.L):
            assert torch.equal(plain.k[i], kv8.k[i]) and torch.equal(plain.v[i], kv8.v[i])
    plain.reset(); kv8.reset()
    kv8.kv_from = 5
    a, b = plain.forward(x), kv8.forward(x)
    assert torch.equal(a[:5], b[:5]) and not torch.equal(a[5:], b[5:])      # queries below the boundary see no MXFP8 row
    assert torch.equal(plain.k[0], kv8.k[0])                                 # the stored rows stay bf16


def test_quantiser_round_trip_is_the_fake_quantiser():
    g = torch.Generator().manual_seed(5)
    x = ac.rb(torch.randn(7, 128, generator=g) * torch.tensor([1e-3, 1.0, 30.0, 448.0, 500.0, 1e4, 0.0])[:, None])
    codes, scales = mx_quantise(x, 32)
    dq = torch.ldexp(codes.view(torch.float8_e4m3fn).float().reshape(7, 4, 32), (scales.to(torch.int32) - 127)[..., None]).reshape(7, 128)
    assert torch.equal(dq, mx_fake_quant(x, 32))
    assert torch.equal(ac.rb(dq), dq)          # the de-quantised values are bf16 values: the kernel's widening is exact


def _cases(KVH, rows):
    return [ac.unshared_case(KVH, rows)] + ac.shared_cases(KVH, rows) + ([ac.grouping_case()] if (KVH, rows) == (4, 32) else [])


@pytest.mark.parametrize("rows", [16, 32, 64, 128, 256])
@pytest.mark.parametrize("KVH", [8, 4, 2])
def test_op_inputs_keep_their_teeth_after_quantisation(KVH, rows):
    worst_mass, dist = 1.0, []
    for case in _cases(KVH, rows):
        for mode in HOST_MODES:
            k8 = kc.Kv8Case(case, mode, rows)
            for (s, h), j in case.spots.items():
                worst_mass = min(worst_mass, float(k8.probs[s][h][j]))
                assert float(k8.probs[s][h][j]) >= 0.99, (mode, s, h, j, float(k8.probs[s][h][j]))
            d = k8.distance()
            dist.append(d)
            assert d >= 1e-2, (KVH, rows, mode, d)
            # the planes: rows [from, pos) quantised, everything else NaN; the bf16 rows there poisoned
            for s in range(case.n):
                f, p = k8.frm[s], case.pos[s]
                if not case.active[s]:
                    assert (k8.k8[s] == kc.NAN8).all() and (k8.v8s[s] == kc.NAN8).all()
                    continue
                assert case.L[s] <= f <= p
                assert (k8.k8[s][:, :f] == kc.NAN8).all() and (k8.k8[s][:, p:] == kc.NAN8).all() and (k8.v8s[s][:, p:] == kc.NAN8).all()
                if p > f:
                    assert float(k8.Kin[s][:, f:p].abs().min()) > 2e4 and float(k8.Vin[s][:, f:p].abs().min()) > 2e4
                assert torch.equal(k8.Kin[s][:, p], case.K[s][:, p])
    print(f"KVH {KVH} rows {rows}: worst spotlight mass {worst_mass:.5f}, distance to the bf16 reference {min(dist):.2e} .. {max(dist):.2e}")


def test_every_boundary_mode_differs_where_it_should():
    case = ac.unshared_case(8, 32)
    frm = {m: kc.boundaries(case, m, 32) for m in kc.MODES}
    s = case.pos.index(319)
    assert [frm[m][s] for m in kc.MODES] == [0, 159, 31, 32, 33, 319]
    s0 = case.pos.index(0)
    assert all(frm[m][s0] == 0 for m in kc.MODES)
    fork = ac.shared_cases(8, 32)[0]
    f2 = kc.boundaries(fork, "L", 32)
    assert f2[0] == max(fork.L) and all(f2[i] == fork.L[i] for i in range(1, fork.n) if fork.active[i])
