"""The decode attention kernels op by op on the MI355X (dtk_op_attn_decode / dtk_op_attn_decode_b) against the float64 softmax of
tests/attn_decode_cases.py, at test_op_attention's bar (rel-L2 < 2e-3, <= 4.01 bf16 ulps): k_attn_decode, k_attn_decode_head,
k_attn_decode_t<256 | 512 | 1024, 128 | 64>, k_attn_combine<128 | 64>, o_proj's PRO_ATTN prologue, k_attn_tail_b (every THREADS / GQ
instantiation) and k_attn_prefix_g.  Random inputs and spotlight inputs (one key holds >= 0.99 of a head's mass, so one key dropped,
counted twice or read from the wrong row cannot pass); rows no kernel may read hold poison."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from oracle.ops import bits_to_f32, f32_to_bits, rb
from tests import attn_decode_cases as ac
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu

RL2, ULPS = 2e-3, 4.01
H = ac.H


@pytest.fixture(scope="module")
def tiny():
    from detikzify_amd.model import load
    return load("detikzify-tiny", synthetic=1234)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _report(got_bits, ref):
    """test_op_attention's measure: max difference in bf16 ulps of the reference (floored at 1 % of the tensor's largest magnitude)
    and rel-L2"""
    got = bits_to_f32(np.ascontiguousarray(got_bits)).reshape(-1)
    ref = rb(torch.as_tensor(ref, dtype=torch.float32)).reshape(-1)
    ulp = torch.clamp(ref.abs(), min=1e-2 * float(ref.abs().max()) + 1e-30) * 2.0 ** -7
    return float(((got - ref).abs() / ulp).max()), rel_l2(got, ref)


class Worst:
    def __init__(self):
        self.w = {}

    def add(self, name, ulps, rl2):
        u, r = self.w.get(name, (0.0, 0.0))
        self.w[name] = (max(u, ulps), max(r, rl2))

    def show(self, what):
        for name, (u, r) in self.w.items():
            print(f"{what} {name}: worst max_ulp {u:.2f} rel_l2 {r:.2e}")


# ------------------------------------------------------------------------------------------ single sequence
def _bits(case):
    if not hasattr(case, "bits"):
        case.bits = tuple(f32_to_bits(x) for x in (case.q, case.K, case.V, case.K2, case.V2))
    return case.bits


def _run_single(model, case, threads, S, mode, variant=-1, other_poison=False):
    qb, kb, vb, kb2, vb2 = _bits(case)
    if other_poison:
        kb, vb = kb2, vb2
    hd, n = case.hd, len(case.positions)
    pos = np.asarray(case.positions, dtype=np.int32)
    out = np.zeros((n, H, hd), dtype=np.uint16)
    pm, pl, po = np.zeros((n, H, S), np.float32), np.zeros((n, H, S), np.float32), np.zeros((n, H, S, hd), np.float32)
    model._check(model.lib.dtk_op_attn_decode(model._ctx, _p(qb), _p(kb), _p(vb), H, case.KVH, hd, ac.T_MAX, _p(pos), n, threads, S, mode,
                                              variant, _p(out), _p(pm), _p(pl), _p(po)), "dtk_op_attn_decode")
    return out, pm, pl, po


def _family(threads, mode, hd):
    if threads == 0:
        return {0: "k_attn_decode + PRO_ATTN", 1: "k_attn_decode in-kernel combine", 2: "k_attn_decode + k_attn_combine<128>",
                3: "k_attn_decode_head"}[mode]
    return f"k_attn_decode_t<{threads}, {hd}> + " + ("PRO_ATTN" if mode == 0 else f"k_attn_combine<{hd}>")


def _empty_splits(threads, hd, S, pos):
    """which splits hold no key at this position"""
    n = pos + 1
    step = ac.tile_rows(threads, hd) if threads else (((n + S - 1) // S) + 15) & ~15
    return [sp * step >= n for sp in range(S)]


def _check_single(model, case, threads, S, mode, worst, label, variant=-1, twice=False):
    out, pm, pl, po = _run_single(model, case, threads, S, mode, variant)
    hd = case.hd
    fam = _family(threads, mode, hd)
    for i, p in enumerate(case.positions):
        ulps, rl2 = _report(out[i], case.ref[i])
        worst.add(fam, ulps, rl2)
        assert rl2 < RL2 and ulps <= ULPS, f"{label} {fam} S {S} variant {variant} pos {p}: max_ulp {ulps:.2f} rel_l2 {rl2:.2e}"
        if mode == 0 and not (threads and S == 1):
            empty = _empty_splits(threads, hd, S, p)
            for sp in range(S):
                assert (pl[i, :, sp] == 0).all() if empty[sp] else (pl[i, :, sp] > 0).all(), f"{label} {fam} S {S} pos {p} split {sp}: l {pl[i, :, sp]}"
            comb = ac.combine_partials(torch.from_numpy(pm[i]), torch.from_numpy(pl[i]), torch.from_numpy(po[i]))
            ulps, rl2 = _report(f32_to_bits(comb.float()), case.ref[i])
            worst.add(fam.split(" + ")[0] + " partials", ulps, rl2)
            assert rl2 < RL2 and ulps <= ULPS, f"{label} {fam} S {S} pos {p} partials in float64: max_ulp {ulps:.2f} rel_l2 {rl2:.2e}"
    if twice:       # other poison above the last position: no bit may move
        out2 = _run_single(model, case, threads, S, mode, variant, other_poison=True)[0]
        assert np.array_equal(out, out2), f"{label} {fam} S {S}: the output depends on rows above the position"
    return out


@pytest.mark.parametrize("hd,KVH", [(128, 8), (128, 2), (64, 8), (64, 2)])
def test_single_sequence_kernels(tiny, hd, KVH):
    """every (threads, mode) the options allow x splits 1, 2, 3, 4, 16 x the 19 positions: random inputs, and spotlight inputs (key
    pos, pos - 1, 0, the first key of the last tile and of the second split; traps at pos + 1; poison above the call's last position,
    run twice with different poison)"""
    model, _ = tiny
    worst = Worst()
    rnd = ac.single_random_case(hd, KVH)
    configs = ac.CONFIGS_128 if hd == 128 else ac.CONFIGS_64
    spot = {}
    for threads, mode in configs:
        for S in ([1] if mode == 3 else ac.SPLITS):
            _check_single(model, rnd, threads, S, mode, worst, "random")
            if (threads, S) not in spot:
                spot[(threads, S)] = ac.single_cases(hd, KVH, threads, S)
            for case in spot[(threads, S)]:
                _check_single(model, case, threads, S, mode, worst, "spotlight", twice=True)
    worst.show(f"attn_decode hd{hd} KVH{KVH}")


@pytest.mark.parametrize("hd", [128, 64])
def test_pro_attn_variants(tiny, hd):
    """o_proj's PRO_ATTN prologue in every tuning variant, on the partials of the tile kernel and of the contiguous-split kernel"""
    model, _ = tiny
    worst = Worst()
    for threads in ((512, 0) if hd == 128 else (512,)):
        rnd, spots = ac.single_random_case(hd, 2), ac.single_cases(hd, 2, threads, 4)
        outs = []
        for variant in range(9):
            outs.append(_check_single(model, rnd, threads, 4, 0, worst, "random", variant=variant))
            for case in spots:
                _check_single(model, case, threads, 4, 0, worst, "spotlight", variant=variant)
        for o in outs[1:]:      # the variants differ in how the GEMV is cut, not in the prologue's arithmetic
            assert np.array_equal(o, outs[0])
    worst.show(f"PRO_ATTN variants 0..8 hd{hd}")


def test_single_sequence_refusals(tiny):
    """what the context's options refuse: contiguous splits at head dim 64, more than 16 splits, the in-kernel combine and the
    one-block-per-head kernel with the tile kernel's thread counts"""
    from detikzify_amd._lib import DtkError
    model, _ = tiny
    for hd, threads, S, mode in ((64, 0, 4, 2), (64, 256, 17, 2), (64, 256, 0, 2), (64, 300, 4, 2), (128, 256, 4, 1), (128, 512, 4, 3)):
        with pytest.raises(DtkError):
            _call_raw(model, ac.single_random_case(hd, 2), threads, S, mode)


def _call_raw(model, case, threads, S, mode):
    qb, kb, vb, _, _ = _bits(case)
    pos = np.asarray([5], dtype=np.int32)
    out = np.zeros((1, H, case.hd), dtype=np.uint16)
    f = np.zeros((H * 16 * case.hd,), np.float32)
    model._check(model.lib.dtk_op_attn_decode(model._ctx, _p(qb), _p(kb), _p(vb), H, case.KVH, case.hd, ac.T_MAX, _p(pos), 1, threads, S, mode,
                                              -1, _p(out), _p(f), _p(f), _p(f)), "dtk_op_attn_decode")


# ------------------------------------------------------------------------------------------ batched
SENTINEL = 0xFFFF


def _bbits(case):
    if not hasattr(case, "bits"):
        case.bits = tuple(f32_to_bits(x) for x in (case.q, case.K, case.V))
    return case.bits


def _run_batch(model, case, nslots, use_prefix, pfx_splits, tail, gqa, nt, layout=None):
    qb, kb, vb = _bbits(case)
    pos, active, src, L = layout if layout is not None else (case.pos, case.active, case.src, case.L)
    T = ac.B_T_MAX
    i32 = lambda a: np.asarray(a[:nslots], dtype=np.int32)
    pos, active, src, L = i32(pos), i32(active), i32(src), i32(L)
    out = np.zeros((nslots, H * 128), dtype=np.uint16)
    model._check(model.lib.dtk_op_attn_decode_b(model._ctx, _p(qb), _p(kb), _p(vb), nslots, H, case.KVH, T, _p(pos), _p(active), _p(src), _p(L),
                                                use_prefix, pfx_splits, tail, gqa, nt, _p(out)), "dtk_op_attn_decode_b")
    return out.reshape(nslots, H, 128)


def _check_batch(model, case, nslots, worst, fam, label, **kw):
    out = _run_batch(model, case, nslots, **kw)
    for s in range(nslots):
        if not case.active[s]:
            assert (out[s] == SENTINEL).all(), f"{label}: the row of idle slot {s} was written"
            continue
        ulps, rl2 = _report(out[s], case.ref[s])
        worst.add(fam, ulps, rl2)
        assert rl2 < RL2 and ulps <= ULPS, (f"{label} {fam} {kw} slot {s} pos {case.pos[s]} src {case.src[s]} L {case.L[s]}: "
                                            f"max_ulp {ulps:.2f} rel_l2 {rl2:.2e}")
    return out


def _gqa_values(KVH):
    return {1: (0,), 2: (0, 1), 4: (0, 1, 2)}[H // KVH]


def _tail_family(tail, KVH, gqa):
    """the instantiation launch_attn_decode_b picks"""
    G = H // KVH
    if G == 4 and gqa == 2:
        return "k_attn_tail_b<256, 2>"
    if G == 4 and gqa:
        return f"k_attn_tail_b<{tail if tail in (64, 128, 512) else 256}, 4>"
    if G == 2 and gqa:
        return f"k_attn_tail_b<{tail if tail in (64, 128) else 256}, 2>"
    return f"k_attn_tail_b<{tail}, 1>"


@pytest.mark.parametrize("tail", [64, 128, 256, 512])
@pytest.mark.parametrize("KVH", [8, 4, 2])
def test_batched_without_sharing(tiny, KVH, tail):
    """16 slots at the positions of the single-sequence list (clipped to T_max - 1), slots 3 and 9 idle: their rows keep the
    sentinel; spotlights on the last key and on the first key of the second and third tile; rows above a slot's position are poison"""
    model, _ = tiny
    worst = Worst()
    case = ac.unshared_case(KVH, tail // 4)
    for gqa in _gqa_values(KVH):
        for nt in (0, 1):
            for use_prefix in (0, 1):      # nothing is shared: the prefix kernel has no group, the tail walks everything
                _check_batch(model, case, 16, worst, _tail_family(tail, KVH, gqa), "unshared", use_prefix=use_prefix, pfx_splits=4, tail=tail,
                             gqa=gqa, nt=nt)
    worst.show(f"attn_decode_b unshared KVH{KVH} tail {tail}")


@pytest.mark.parametrize("tail", [64, 128, 256, 512])
@pytest.mark.parametrize("KVH", [8, 4, 2])
def test_batched_shared_prefix(tiny, KVH, tail):
    """forks of slot 0 with share_len 3 (below the grouping threshold), 4, 63, 64, 65, 153, 256 x private lengths 1, 2, ROWS - 1,
    ROWS, ROWS + 1, 2 ROWS + 1, 3 ROWS + 1; the fork's own rows below share_len are poison; spotlights on keys 0 and L - 1 (the
    source's rows; the source's row L is a trap), L and the last key (the fork's own); with and without k_attn_prefix_g, 1..4 key splits"""
    model, _ = tiny
    worst = Worst()
    cases = ac.shared_cases(KVH, tail // 4)
    for gqa in _gqa_values(KVH):
        fam = _tail_family(tail, KVH, gqa)
        for nt in (0, 1):
            for use_prefix, splits in ((0, 1), (1, 1), (1, 2), (1, 3), (1, 4)):
                name = fam + (f" + k_attn_prefix_g" if use_prefix else "")
                for case in cases:
                    _check_batch(model, case, 16, worst, name, "shared", use_prefix=use_prefix, pfx_splits=splits, tail=tail, gqa=gqa, nt=nt)
    worst.show(f"attn_decode_b shared KVH{KVH} tail {tail}")


def test_batched_grouping(tiny):
    """64 slots: a source with 17 forks (a group of 16 and a singleton), one with 2, one that decodes itself, slots that share nothing;
    a fork's bits do not depend on its company"""
    model, _ = tiny
    worst = Worst()
    case = ac.grouping_case()
    kw = dict(use_prefix=1, pfx_splits=4, tail=128, gqa=1, nt=1)
    out = _check_batch(model, case, 64, worst, "k_attn_tail_b<128, 2> + k_attn_prefix_g", "grouping", **kw)
    _check_batch(model, case, 64, worst, "k_attn_tail_b<128, 2>", "grouping", **dict(kw, use_prefix=0))
    alone = _run_batch(model, case, 16, layout=ac.sub_case(case, 16, 5), **kw)
    assert np.array_equal(alone[5], out[5]) and (np.delete(alone, 5, axis=0) == SENTINEL).all()
    alone = _run_batch(model, case, 32, layout=ac.sub_case(case, 32, 17), **kw)      # the singleton of the 17
    assert np.array_equal(alone[17], out[17])
    worst.show("attn_decode_b grouping (64 slots)")


@pytest.mark.parametrize("tail", [512, 1024])
@pytest.mark.parametrize("nslots", [1, 2, 4])
def test_batched_multi_vector_grid(tiny, nslots, tail):
    """the <= 4-slot step's grid: k_attn_tail_b<512 | 1024> with 1, 2 and 4 slots, no prefix kernel; forks still read their source"""
    model, _ = tiny
    worst = Worst()
    rows = tail // 4
    for KVH in (8, 2):
        layouts = [[{"pos": 319}, {"pos": rows}, {"pos": 0}, {"pos": min(2 * rows - 1, 319)}][:nslots]]
        if nslots > 1:
            layouts.append([{"pos": 319}, {"pos": min(64 + rows, 319), "src": 0, "L": 64}, {"pos": 3, "src": 0, "L": 3}, {"pos": 255 + 1, "src": 0, "L": 255}][:nslots])
        for i, slots in enumerate(layouts):
            case = ac.BatchCase(KVH, slots, seed=50 * nslots + KVH + i, rows=rows)
            for gqa in (0, 1):
                for nt in (0, 1):
                    _check_batch(model, case, nslots, worst, _tail_family(tail, KVH, gqa), "multi-vector", use_prefix=0, pfx_splits=4, tail=tail,
                                 gqa=gqa, nt=nt)
    worst.show(f"attn_decode_b multi-vector nslots {nslots} tail {tail}")
