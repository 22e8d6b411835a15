"""The two selections of dtk_set_option "top_logprobs" on bare rows (dtk_op_top_logits): k_top_logits (kernel 1) and k_top_slice +
k_top_merge (kernel 2) against a numpy lexsort of (-z, id).  Ids and the bits of z must be exactly equal, for either kernel and
between the two.  The shapes are the smallest at which the sliced pair can go wrong: one element, V = k, several slices with a
ragged last one, one full slice, a last slice shorter than k, more than one row, and the v2 vocabulary at the default slice."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOP = 8
POISON_ID, POISON_Z = 0x5A5A5A5A, np.float32(-12345.5)
# (V, L of kernel 2, rows of the plain call)
SHAPES = [(1, 8192, 1), (8, 8192, 1), (300, 128, 1), (8192, 8192, 1), (8192 + 5, 8192, 1), (2 * 8192 + 1037, 8192, 3), (128256, 8192, 2)]


@pytest.fixture(scope="module")
def ctx():
    from detikzify_amd.model import load
    return load("detikzify-tiny", synthetic=1234)[0]


def reference(rows, k):
    """per row the first k of the vocabulary ordered by z descending, id ascending on ties: ids and z"""
    ids = np.empty((len(rows), k), np.int32)
    for r, z in enumerate(rows):
        order = np.lexsort((np.arange(z.size), -z.astype(np.float64)))[:k]
        ids[r] = order
    return ids, np.take_along_axis(np.asarray(rows), ids.astype(np.int64), axis=1)


_ROWS = {}


def content_rows(V, L):
    """the rows every shape is tried with (built once per shape, read-only): random normal | one constant | the 8 largest one per
    slice | the 8 largest all in the last, ragged slice | equal maxima at the last index of slice s and the first of slice s + 1 |
    -inf everywhere but at three places (fewer finite values than k = 8)"""
    if (V, L) not in _ROWS:
        g = np.random.default_rng(V * 31 + L)
        n = -(-V // L)
        last = (n - 1) * L                                  # first index of the last slice
        normal = lambda: g.standard_normal(V).astype(np.float32)
        const = np.full(V, np.float32(0.75))
        spread = normal()
        for j in range(min(TOP, V)):                        # one per slice (round-robin where there are fewer slices than 8)
            s = j % n
            lo, hi = s * L, min(V, (s + 1) * L)
            spread[lo + ((hi - lo) // 2 + j // n) % (hi - lo)] = np.float32(100 + j)
        tail = normal()
        for j in range(min(TOP, V - last)):
            tail[V - 1 - j] = np.float32(200 + (j * 5) % 7)      # (with equal values among them)
        edge = normal()
        for s in range(n - 1):
            edge[(s + 1) * L - 1] = edge[(s + 1) * L] = np.float32(50)
        if n == 1:
            edge[0] = edge[V - 1] = np.float32(50)
        holes = np.full(V, -np.inf, np.float32)
        for j, at in enumerate(sorted({V - 1, V // 2, min(V - 1, L)})[: max(0, min(3, V - 1))]):
            holes[at] = np.float32(-3.5 + j)
        rows = np.stack([normal(), const, spread, tail, edge, holes])
        rows.setflags(write=False)
        _ROWS[(V, L)] = rows
    return _ROWS[(V, L)]


def run(ctx, rows, k, kernel, L, active=None, forced=None):
    rows = np.ascontiguousarray(rows, np.float32)
    R, V = rows.shape
    ids = np.full((R, TOP), POISON_ID, np.int32)
    z = np.full((R, TOP), POISON_Z, np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    a = None if active is None else np.asarray(active, np.int32)
    f = None if forced is None else np.asarray(forced, np.int32)
    ctx._check(ctx.lib.dtk_op_top_logits(ctx._ctx, p(rows), R, V, k, kernel, L, p(a), p(f), p(ids), p(z)), "dtk_op_top_logits")
    return ids, z


def check(ids, z, want_ids, want_z, k, what):
    assert np.array_equal(ids[:, :k], want_ids), (what, np.argwhere(ids[:, :k] != want_ids)[:4])
    assert np.array_equal(z[:, :k].view(np.uint32), want_z.view(np.uint32)), what
    assert (ids[:, k:] == POISON_ID).all() and (z[:, k:] == POISON_Z).all(), (what, "entries >= k were written")


CASES = [(V, L, R, k) for V, L, R in SHAPES for k in (1, 3, 8) if k <= V]


@pytest.mark.parametrize("V,L,R,k", CASES, ids=[f"V{v}-L{l}-k{k}" for v, l, _, k in CASES])
def test_both_kernels_against_a_lexsort(ctx, V, L, R, k):
    rows = content_rows(V, L)
    want_ids, want_z = reference(rows, k)
    got = {}
    for kernel in (1, 2):
        got[kernel] = run(ctx, rows, k, kernel, L)
        check(*got[kernel], want_ids, want_z, k, (V, L, k, kernel))
    assert got[1][0].tobytes() == got[2][0].tobytes() and got[1][1].tobytes() == got[2][1].tobytes()
    # the constant row: every tie resolves to the lowest ids, across slice boundaries
    assert got[2][0][1, :k].tolist() == list(range(k))
    # the plain call of the shape: R random rows, nobody inactive or forced
    plain = np.random.default_rng(V + k).standard_normal((R, V)).astype(np.float32)
    pw = reference(plain, k)
    for kernel in (1, 2):
        check(*run(ctx, plain, k, kernel, L), *pw, k, (V, L, k, kernel, "plain"))


@pytest.mark.parametrize("V,L", [(300, 128), (8192 + 5, 8192)])
def test_inactive_and_forced_rows(ctx, V, L):
    rows = content_rows(V, L)
    k = min(3, V)
    active, forced = [1, 0, 1, 1, 0, 1], [0, 0, 1, 0, 1, 0]
    want_ids, want_z = reference(rows, k)
    for kernel in (1, 2):
        ids, z = run(ctx, rows, k, kernel, L, active, forced)
        for r in range(len(rows)):
            if not active[r]:           # an inactive row keeps the caller's bytes (forced or not)
                assert (ids[r] == POISON_ID).all() and (z[r] == POISON_Z).all(), (kernel, r)
            elif forced[r]:             # a forced row: (-1, NaN) in its first k entries, nothing behind them
                assert (ids[r, :k] == -1).all() and np.isnan(z[r, :k]).all(), (kernel, r)
                assert (ids[r, k:] == POISON_ID).all() and (z[r, k:] == POISON_Z).all(), (kernel, r)
            else:
                check(ids[r:r + 1], z[r:r + 1], want_ids[r:r + 1], want_z[r:r + 1], k, (kernel, r))


def test_bad_arguments_are_refused(ctx):
    rows = np.zeros((1, 300), np.float32)
    ids, z = np.zeros((1, TOP), np.int32), np.zeros((1, TOP), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda R, V, k, kernel, L: ctx.lib.dtk_op_top_logits(ctx._ctx, p(rows), R, V, k, kernel, L, None, None, p(ids), p(z))
    assert call(1, 300, 3, 2, 128) == 0 and call(1, 300, 3, 1, 0) == 0          # (kernel 1 does not look at L)
    for R, V, k, kernel, L in ((1, 300, 3, 2, 0), (1, 300, 3, 2, 8193), (1, 300, 3, 2, 9), (1, 300, 9, 1, 128), (1, 2, 3, 1, 128),
                               (1, 300, 0, 2, 128), (1, 300, 3, 0, 128), (1, 300, 3, 3, 128), (0, 300, 3, 1, 128), (65, 300, 3, 1, 128)):
        assert call(R, V, k, kernel, L) == -1, (R, V, k, kernel, L)              # (L = 9: 34 slices, more than 32)
    for name, bad in (("top_kernel", 3), ("top_kernel", -1), ("top_slice", 0), ("top_slice", 8193), ("top_slice", 1)):
        assert ctx.lib.dtk_set_option(ctx._ctx, name.encode(), bad) == -1, (name, bad)
