"""No GPU: (1) the RMSNorm prologue's fold of k_gemv mirrored in float32 numpy (tests/w13_fold.py) - the 13-bit shapes of 8 and 16 waves
fold the sum of squares as a 4-wave block does, and at the pinned seeds of tests/w13_fold.NORM_CASES that fold and the block's own give
another `inv`, so tests/test_gpu_w13_shapes.py cannot pass on a kernel that ignores the parameter; (2) w13.h's rule for the device's
row byte (hb | 0x80 where a weight of the row has e >> 1 == 0); (3) the host packer's output, unchanged: a recorded digest."""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np
import pytest

from detikzify_amd import _lib
from tests import w13_fold as wf

ZROW = 0x80


@pytest.fixture(scope="module")
def lib():
    return _lib.load_library()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------ the fold
@pytest.mark.parametrize("fw", (4, 8, 16))
def test_mirror_is_the_sum_of_squares(fw):
    """the mirror against float64, both forms: a fold of K = 4096 values is within a few ulps of the exact sum"""
    rng = np.random.default_rng(fw)
    for K in (72, 520, 4096, 4104, 11008):
        x = (rng.standard_normal(K).astype(np.float32).view(np.uint32) & 0xFFFF0000).view(np.float32)
        exact = float((x.astype(np.float64) ** 2).sum())
        forms = [None] + ([True, False] if K // 8 <= 2 * fw * 64 else [])
        tots = [float(wf.fold_tot(x, fw, f)) for f in forms]
        assert all(abs(t - exact) <= 16 * 2.0 ** -24 * exact for t in tots), (K, tots, exact)
        assert len(set(tots)) == 1, (K, tots)          # a thread holds the same chunks in the same order in either form


def test_first_threads_of_a_larger_block_fold_as_the_small_block():
    """what FW means: thread t < FW * 64 holds chunks t, t + FW * 64, ... whatever the block's size, so the fold is a function of FW
    alone; the mirror takes no block size at all, and the form follows FW (K8 <= 2 * FW * 64), not the block"""
    for role, kw, seed in wf.NORM_CASES:
        x = wf.case_x(role, kw, seed)
        K8 = x.size // 8
        assert (K8 <= 512) == (kw["K"] == 4096)        # K = 4096 takes the one-pass form of a 4-wave fold, K = 4104 the strided one
        assert wf.inv_bits(x, 4, one_pass=False) == wf.inv_bits(x, 4)


@pytest.mark.parametrize("i", range(len(wf.NORM_CASES)), ids=lambda i: f"{wf.gc.EPI_NAME[wf.NORM_CASES[i][0][1]]}-K{wf.NORM_CASES[i][1]['K']}-hd{wf.NORM_CASES[i][1].get('hd', 128)}")
def test_pinned_seed_tells_the_folds_apart(i):
    role, kw, seed = wf.NORM_CASES[i]
    x = wf.case_x(role, kw, seed)
    if kw.get("H", 0) <= 2 or i == 6:                   # the x is the case's own (one of the two large matrices is enough)
        assert np.array_equal(wf.gc.Case(role[0], role[1], "bf16", seed=seed, **kw).x.numpy().astype(np.float32), x)
    assert wf.packable(role, kw, seed)                  # or the op would run the bf16 kernel and the GPU test would say so
    inv = {fw: wf.inv_bits(x, fw) for fw in (4, 8, 16)}
    print(f"K {kw['K']} seed {seed}: inv bits " + ", ".join(f"{fw} waves {b:#010x}" for fw, b in inv.items()))
    assert inv[4] != inv[8] and inv[4] != inv[16], inv


def test_both_K_have_a_pinned_seed():
    assert {kw["K"] for _, kw, _ in wf.NORM_CASES} == {4096, 4104}
    for role, new in wf.NEW.items():
        assert all(wf.TABLE13[role][v][4] == 4 and wf.TABLE13[role][v][2] in (8, 16) and wf.TABLE13[role][v][3] for v in new)


# ------------------------------------------------------------------------------------------ the row byte
def _row(K, hb, rng):
    q = rng.integers(max(hb - 14, 1), hb + 1, K)
    w = (rng.integers(0, 2, K) << 15) | (q << 8) | rng.integers(0, 256, K)
    w[rng.integers(0, K)] = (hb << 8) | 0x12
    return w.astype(np.uint16)


def _bytes(lib, W):
    W = np.ascontiguousarray(W, dtype=np.uint16)
    out = np.full(W.shape[0], 0x55, np.uint8)
    assert lib.dtk_w13_row_bytes_host(_p(W), W.shape[0], W.shape[1], _p(out)) == 0
    return out


@pytest.mark.parametrize("K", (8, 520, 1544))
def test_row_byte_rule(lib, K):
    rng = np.random.default_rng(K)
    for hb in (1, 15, 16, 17, 63, 127):
        lo = max(hb - 15, 0)
        base = _row(K, hb, rng)
        planted = {"+0": 0x0000, "-0": 0x8000, "denormal": 0x0001, "-denormal": 0x807F, "e=1": 0x00C5, "-e=1": 0x80FF}
        rows, want = [base], [hb]
        for pat in planted.values():
            for k in (0, K // 2, K - 1):
                r = base.copy()
                r[k] = pat
                if ((r >> 8) & 0x7F).max() == hb:      # (K = 8 can lose its largest weight to the plant)
                    rows.append(r)
                    want.append(hb | ZROW)
        if hb >= 2:                                      # the smallest e >> 1 a row can hold beside zero codes: lo + 1 (code 1), not flagged
            r = base.copy()
            r[K // 2] = (max(lo + 1, 1) << 8) | 0x7F
            r[0] = (hb << 8) | 0x01
            rows.append(r)
            want.append(hb)
            assert int(((r >> 8) & 0x7F).min()) == max(lo + 1, 1)
        got = _bytes(lib, np.stack(rows))
        assert np.array_equal(got, np.array(want, np.uint8)), (K, hb, got, want)
        # the host packer's hb stays the plain byte, and the planes decode to the rows under either byte
        W = np.stack(rows)
        rb = lib.dtk_w13_row_bytes(K)
        planes, hbs, bad = np.zeros((len(rows), rb), np.uint8), np.zeros(len(rows), np.uint8), np.zeros(len(rows), np.int32)
        assert lib.dtk_w13_pack_host(_p(W), len(rows), K, _p(planes), _p(hbs), _p(bad)) == 0
        assert not bad.any() and np.array_equal(hbs, np.full(len(rows), hb, np.uint8))
        for byte in (hbs, got):
            back = np.zeros_like(W)
            assert lib.dtk_w13_unpack_host(_p(planes), _p(np.ascontiguousarray(byte)), len(rows), K, _p(back)) == 0
            assert np.array_equal(back, W)


def test_row_byte_refusals(lib):
    W = np.zeros((1, 12), np.uint16)
    assert lib.dtk_w13_row_bytes_host(_p(W), 1, 12, _p(W)) != 0
    assert lib.dtk_w13_row_bytes_host(None, 1, 8, _p(W)) != 0
    assert lib.dtk_w13_flagged_rows(None, 0) == -1


# ------------------------------------------------------------------------------------------ the packer's output is what it was
def digest_matrix():
    rng = np.random.default_rng(1032)
    W = (rng.standard_normal((5, 1032)).astype(np.float32) * np.float32(0.02)).view(np.uint32) >> 16
    W = W.astype(np.uint16)
    W[2, 7] = 0x8000
    W[3, 1031] = 0x00C5
    W[4, 512] = 0x0001
    return W


DIGEST = "51012695c1c406868574d0f0fb4e709909030dce9ee3fb37a1e64a985ad25d9e"


def test_host_packer_output_is_unchanged(lib):
    """sha256 over planes, hb and bad of dtk_w13_pack_host for one K = 1032 matrix, recorded from the commit before the row byte's flag"""
    W = digest_matrix()
    rb = lib.dtk_w13_row_bytes(1032)
    planes, hb, bad = np.full((5, rb), 0xA5, np.uint8), np.zeros(5, np.uint8), np.zeros(5, np.int32)
    assert lib.dtk_w13_pack_host(_p(W), 5, 1032, _p(planes), _p(hb), _p(bad)) == 0
    assert hb.max() < ZROW
    h = hashlib.sha256(planes.tobytes() + hb.tobytes() + bad.tobytes()).hexdigest()
    assert h == DIGEST, h
