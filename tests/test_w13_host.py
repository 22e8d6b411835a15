"""csrc/w13.h's host packer through dtk_w13_pack_host / dtk_w13_unpack_host (no GPU): bf16 rows -> 13-bit planes -> the same bits.

A row's window is e >> 1 in [hb - 14, hb] (hb = the row's largest e >> 1) plus e >> 1 == 0; a weight below it makes the row unpackable,
which the packer reports (bad[r] > 0) instead of altering it.  tools/w13_selftest.cpp runs the same code under the host sanitizers."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from detikzify_amd import _lib

KS = (8, 72, 512, 520, 1544)          # one ragged unit, a whole unit, a unit + one chunk, one sign block + a ragged unit


@pytest.fixture(scope="module")
def lib():
    return _lib.load_library()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pack(lib, W):
    W = np.ascontiguousarray(W, dtype=np.uint16)
    N, K = W.shape
    rb = lib.dtk_w13_row_bytes(K)
    assert rb == ((K // 8 + 127) // 128) * 1536 + (((K // 8 + 127) // 128 + 1) // 2) * 256
    planes, hb, bad = np.full((N, rb), 0xA5, np.uint8), np.zeros(N, np.uint8), np.zeros(N, np.int32)
    assert lib.dtk_w13_pack_host(_p(W), N, K, _p(planes), _p(hb), _p(bad)) == 0
    return planes, hb, bad


def unpack(lib, planes, hb, K):
    N = planes.shape[0]
    out = np.zeros((N, K), np.uint16)
    assert lib.dtk_w13_unpack_host(_p(planes), _p(hb), N, K, _p(out)) == 0
    return out


def roundtrip(lib, W):
    planes, hb, bad = pack(lib, W)
    assert not bad.any(), bad
    assert np.array_equal(hb, ((W >> 8) & 0x7F).max(1))
    back = unpack(lib, planes, hb, W.shape[1])
    assert np.array_equal(back, W)
    return planes


def window_patterns(hb):
    """all 65536 bf16 patterns restricted to the window of a row whose largest e >> 1 is hb"""
    p = np.arange(65536, dtype=np.uint32)
    q = (p >> 8) & 0x7F
    return p[(q == 0) | ((q >= max(hb - 14, 1)) & (q <= hb))].astype(np.uint16)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("hb", (0, 1, 14, 15, 16, 63, 126, 127))
def test_every_pattern_of_a_window_round_trips(lib, K, hb):
    pats = window_patterns(hb)
    assert len(pats) == 512 * (1 + min(hb, 15))
    rng = np.random.default_rng(1000 * K + hb)
    n = -(-len(pats) // K) + 1
    W = np.concatenate([rng.permutation(pats), rng.choice(pats, n * K - len(pats))]).reshape(n, K)
    W[:, 0] = (hb << 8) | 0x12                   # every row has the maximum, so every row has this window
    roundtrip(lib, W)


@pytest.mark.parametrize("K", KS)
def test_zeros_denormals_and_e1_among_normal_weights(lib, K):
    rng = np.random.default_rng(K)
    normal = ((rng.integers(0, 2, (6, K)) << 15) | (rng.integers(100, 115, (6, K)) << 8) | rng.integers(0, 256, (6, K))).astype(np.uint16)
    tiny = np.array([0x0000, 0x8000, 0x0001, 0x807F, 0x0080, 0x80FF, 0x0040], np.uint16)      # +-0, denormals, e = 1
    W = normal.copy()
    W[rng.integers(0, 2, W.shape).astype(bool)] = 0                                            # half of it exact zeros
    W[:, ::3] = rng.choice(tiny, W[:, ::3].shape)
    W[:, -1] = 114 << 8
    roundtrip(lib, W)


@pytest.mark.parametrize("K", KS)
def test_widest_window_and_one_value_beyond_it(lib, K):
    rng = np.random.default_rng(7 * K)
    hb = 100
    q = rng.integers(hb - 14, hb + 1, (4, K))
    W = ((rng.integers(0, 2, q.shape) << 15) | (q << 8) | rng.integers(0, 256, q.shape)).astype(np.uint16)
    W[:, 0], W[:, K - 1] = (hb << 8) | 0xFF, ((hb - 14) << 8) | 0x00           # both ends of the window in every row
    roundtrip(lib, W)
    V = W.copy()
    V[2, K // 2] = ((hb - 15) << 8) | 0xFF                                       # the largest value below the window
    planes, hbs, bad = pack(lib, V)
    assert bad.tolist() == [0, 0, 1, 0]
    back = unpack(lib, planes, hbs, K)
    assert np.array_equal(back[[0, 1, 3]], V[[0, 1, 3]])                          # the other rows are untouched by the bad one
    assert back[2, K // 2] == 0 and np.array_equal(np.delete(back[2], K // 2), np.delete(V[2], K // 2))   # reported, and not another value


@pytest.mark.parametrize("K", KS)
def test_inf_and_nan_are_exact_or_reported(lib, K):
    rng = np.random.default_rng(3 * K)
    special = np.array([0x7F80, 0xFF80, 0x7FC0, 0xFFFF, 0x7F81], np.uint16)
    for q_lo, packable in ((113, True), (112, False), (60, False)):
        q = rng.integers(q_lo, 127, (2, K))
        W = ((q << 8) | rng.integers(0, 256, q.shape)).astype(np.uint16)
        W[:, : min(K, 5)] = special[: min(K, 5)]
        W[:, -1] = (q_lo << 8) | 1
        planes, hb, bad = pack(lib, W)
        assert (hb == 127).all()
        if packable:
            assert not bad.any() and np.array_equal(unpack(lib, planes, hb, K), W)
        else:
            qs = (W >> 8) & 0x7F
            assert np.array_equal(bad, ((qs > 0) & (qs < 113)).sum(1)) and (bad > 0).all()          # reported, weight by weight


@pytest.mark.parametrize("K", KS)
def test_padding_is_zero_and_layout_is_the_documented_one(lib, K):
    """a single non-zero weight at k lands where w13.h's header says; everything else of the row, the padding included, is zero"""
    for k in sorted({0, 3, 4, 7, K - 1, K // 2, min(K - 1, 519), min(K - 1, 1031)}):
        W = np.zeros((1, K), np.uint16)
        W[0, k] = 0x8000 | (0x3F << 8) | 0xC3          # negative, e >> 1 = 63 (code 15 under lo = 48), low byte 0xC3
        row = roundtrip(lib, W)[0]
        c, e = k // 8, k % 8
        J2 = (K // 8 + 127) // 128
        lane, unit, half, it = c % 64, c // 128, (c // 64) % 2, (c // 64) % 4
        want = np.zeros_like(row)
        want[(unit * 64 + lane) * 16 + half * 8 + e] = 0xC3
        want[J2 * 1024 + (unit * 64 + lane) * 8 + half * 4 + e % 4] = 15 << (4 * (e // 4))
        want[J2 * 1536 + ((c // 256) * 64 + lane) * 4 + e % 4] = 1 << (2 * it + e // 4)
        assert np.array_equal(row, want), k


def test_bad_arguments(lib):
    assert lib.dtk_w13_row_bytes(12) == -1 and lib.dtk_w13_row_bytes(0) == -1
    W = np.zeros((1, 8), np.uint16)
    assert lib.dtk_w13_pack_host(_p(W), 1, 12, _p(W), _p(W), _p(W)) != 0
    assert lib.dtk_w13_op_bad_rows(None) == -1
