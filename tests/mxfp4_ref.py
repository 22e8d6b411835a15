"""
OCP MXFP4 reference (numpy, float64): the rule weight_format="mxfp4" quantises by, restated without the kernel's bit tricks.

A row of K weights is cut into blocks of 32 along K (the last one may be ragged).  A block's scale is 2^e with e the smallest
integer at which amax * 2^-e <= 6 (the largest E2M1 magnitude); an all-zero block takes e = 0; e is kept >= -126 (a normal fp32
scale; bf16 weights never get there).  A code is the round-to-nearest-even of w * 2^-e onto the E2M1 grid
{0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties going to the value whose code has an even mantissa bit (codes 0, 2, 4, 6 = 0, 1, 2, 4), sign in
bit 3.  Byte i of a block holds weight 2i in its low nibble and 2i + 1 in its high one; a ragged block is padded with zero codes.
"""
from __future__ import annotations

import math

import numpy as np

GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
BLOCK = 32


def block_exp(amax: float) -> int:
    """smallest e with amax * 2^-e <= 6, by search (the kernel reads it from the bits of amax: E - 2, + 1 if the mantissa > 1.5)"""
    if amax == 0.0:
        return 0
    m, ex = math.frexp(amax)            # amax = m * 2^ex, 0.5 <= m < 1
    e = ex - 4                          # 2^(ex-1) <= amax < 2^ex: candidates ex - 4 .. ex - 2
    while amax * 2.0 ** -e > 6.0:
        e += 1
    while amax * 2.0 ** -(e - 1) <= 6.0:
        e -= 1
    return max(-126, min(126, e))


def e2m1_code(v: float) -> int:
    """code 0..7 of the grid value nearest to v in [0, 6]; a tie goes to the even code"""
    best, best_d = 0, None
    for c, g in enumerate(GRID):
        d = abs(v - g)
        if best_d is None or d < best_d or (d == best_d and c % 2 == 0):
            best, best_d = c, d
    return best


def quantise(W):
    """W [N][K] (anything numpy takes; values are used as float64) -> (codes uint8 [N][ceil(K/32)*16], scales uint8 [N][ceil(K/32)],
    W_eff float64 [N][K])"""
    W = np.asarray(W, dtype=np.float64)
    assert W.ndim == 2
    N, K = W.shape
    KC = (K + BLOCK - 1) // BLOCK
    codes = np.zeros((N, KC * 16), dtype=np.uint8)
    scales = np.zeros((N, KC), dtype=np.uint8)
    W_eff = np.zeros_like(W)
    # vectorised over rows, block by block (the per-element rule is e2m1_code: checked against this path by the host tests)
    mids = (GRID[:-1] + GRID[1:]) / 2           # 0.25 0.75 1.25 1.75 2.5 3.5 5
    up_on_tie = np.array([False, True, False, True, False, True, False])      # a tie at mids[i] lies between codes i and i + 1: up iff i + 1 is even
    for c in range(KC):
        blk = W[:, c * BLOCK:min(K, (c + 1) * BLOCK)]
        amax = np.abs(blk).max(axis=1)
        e = np.array([block_exp(float(a)) for a in amax], dtype=np.int64)
        v = np.abs(blk) * np.exp2(-e.astype(np.float64))[:, None]
        assert float(v.max(initial=0.0)) <= 6.0
        code = np.zeros(blk.shape, dtype=np.int64)
        for i in range(7):
            code += (v >= mids[i]) if up_on_tie[i] else (v > mids[i])
        full = code | (np.signbit(blk).astype(np.int64) << 3)
        W_eff[:, c * BLOCK:c * BLOCK + blk.shape[1]] = np.where(np.signbit(blk), -1.0, 1.0) * GRID[code] * np.exp2(e.astype(np.float64))[:, None]
        padded = np.zeros((N, BLOCK), dtype=np.int64)
        padded[:, :blk.shape[1]] = full
        codes[:, c * 16:(c + 1) * 16] = (padded[:, 0::2] | (padded[:, 1::2] << 4)).astype(np.uint8)
        scales[:, c] = (e + 127).astype(np.uint8)
    return codes, scales, W_eff


def dequantise(codes, scales, K: int):
    """the inverse map of the two arrays alone (what a kernel that reads them must compute with)"""
    codes, scales = np.asarray(codes), np.asarray(scales)
    N, KC = scales.shape
    nib = np.zeros((N, KC * BLOCK), dtype=np.int64)
    nib[:, 0::2] = codes & 15
    nib[:, 1::2] = codes >> 4
    val = np.where(nib & 8, -1.0, 1.0) * GRID[nib & 7] * np.repeat(np.exp2(scales.astype(np.float64) - 127.0), BLOCK, axis=1)
    return val[:, :K]


def gemv_ref(W_eff, x):
    """y = W_eff . x in float64"""
    return np.asarray(W_eff, dtype=np.float64) @ np.asarray(x, dtype=np.float64)
