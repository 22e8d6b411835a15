"""k_attn_tail_b<THREADS, GQ, KV8 = true> op by op on the MI355X (dtk_op_attn_decode_b8) against the float64 softmax over the
DE-QUANTISED rows (tests/kv8_cases.py), at tests/test_gpu_attn_decode.py's own bar: rel-L2 < 2e-3, <= 4.01 bf16 ulps.  The bf16 rows
the kernel must read from the shadow are poison, the shadow rows it must not read are NaN; after the call the shadow holds
mx_quantise of row pos of every active (slot, kv head) bit for bit and not one other byte of it has changed.  The bf16 caches are
operands of the op (const host arrays, uploaded): dtk_op_attn_decode_b8 itself reads both back after the launch, compares every byte with
what was uploaded and fails with DTK_ERR_STATE naming the first changed element — so every call below that returns also asserts that
no bf16 byte changed (model._check raises on that code)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import attn_decode_cases as ac
from tests import kv8_cases as kc
from tests.test_gpu_attn_decode import H, RL2, SENTINEL, ULPS, Worst, _gqa_values, _p, _report, _tail_family

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    from detikzify_amd.model import load
    return load("detikzify-tiny", synthetic=1234)


def _run8(model, k8, nslots, use_prefix, pfx_splits, tail, gqa, nt, active=None):
    case = k8.case
    qb, kb, vb = k8.bits()
    T = ac.B_T_MAX
    i32 = lambda a: np.asarray(a[:nslots], dtype=np.int32)
    act = i32(case.active if active is None else active)
    pos, src, L, frm = i32(case.pos), i32(case.src), i32(case.L), i32(k8.frm)
    planes = [np.ascontiguousarray(x[:nslots]).copy() for x in (k8.k8, k8.k8s, k8.v8, k8.v8s)]
    out = np.zeros((nslots, H * 128), dtype=np.uint16)
    model._check(model.lib.dtk_op_attn_decode_b8(model._ctx, _p(qb), _p(kb), _p(vb), nslots, H, case.KVH, T, _p(pos), _p(act), _p(src), _p(L),
                                                 _p(frm), _p(planes[0]), _p(planes[1]), _p(planes[2]), _p(planes[3]),
                                                 use_prefix, pfx_splits, tail, gqa, nt, _p(out)), "dtk_op_attn_decode_b8")
    return out.reshape(nslots, H, 128), planes, act


def _check8(model, k8, nslots, worst, fam, label, active=None, **kw):
    case = k8.case
    out, planes, act = _run8(model, k8, nslots, active=active, **kw)
    want = [np.ascontiguousarray(x[:nslots]).copy() for x in (k8.k8, k8.k8s, k8.v8, k8.v8s)]
    for s in range(nslots):
        if not act[s]:
            assert (out[s] == SENTINEL).all(), f"{label}: the row of idle slot {s} was written"
            continue
        p = case.pos[s]
        want[0][s][:, p], want[1][s][:, p] = k8.want[(s, "k")]
        want[2][s][:, p], want[3][s][:, p] = k8.want[(s, "v")]
        ulps, rl2 = _report(out[s], k8.ref[s])
        worst.add(fam, ulps, rl2)
        assert rl2 < RL2 and ulps <= ULPS, (f"{label} {fam} {kw} from {k8.mode} slot {s} pos {p} src {case.src[s]} L {case.L[s]} kv8_from {k8.frm[s]}: "
                                            f"max_ulp {ulps:.2f} rel_l2 {rl2:.2e}")
    for name, got, exp in zip(("K codes", "K scales", "V codes", "V scales"), planes, want):
        if not np.array_equal(got, exp):
            bad = np.argwhere(got != exp)[0]
            raise AssertionError(f"{label} {fam} {kw} from {k8.mode}: shadow {name} differ first at (slot, kv head, row, byte) {bad.tolist()}: "
                                 f"{got[tuple(bad)]:#x}, expected {exp[tuple(bad)]:#x} (pos {case.pos[bad[0]]}, kv8_from {k8.frm[bad[0]]})")
    return out


def _configs(mode, prefix_ok=True):
    """(nt, use_prefix, splits): everything for the boundary at L and inside the range, the two ends of it for the other modes"""
    if mode in ("L", "mid"):
        return [(nt, up, sp) for nt in (0, 1) for up, sp in (((0, 1), (1, 1), (1, 4)) if prefix_ok else ((0, 1),))]
    return [(1, 1, 4), (0, 0, 1)] if prefix_ok else [(1, 0, 1), (0, 0, 1)]


@pytest.mark.parametrize("tail", [64, 128, 256, 512])
@pytest.mark.parametrize("KVH", [8, 4, 2])
def test_kv8_without_sharing(tiny, KVH, tail):
    """16 slots, two idle; every boundary mode: the whole context from the shadow, half of it, a tile edge and its neighbours, only
    the new row"""
    model, _ = tiny
    worst = Worst()
    case = ac.unshared_case(KVH, tail // 4)
    for mode in kc.MODES:
        k8 = kc.Kv8Case(case, mode, tail // 4)
        for gqa in _gqa_values(KVH):
            for nt, up, sp in _configs(mode):
                _check8(model, k8, 16, worst, _tail_family(tail, KVH, gqa) + " KV8", "unshared", use_prefix=up, pfx_splits=sp, tail=tail, gqa=gqa, nt=nt)
    worst.show(f"attn_decode_b8 unshared KVH{KVH} tail {tail}")


@pytest.mark.parametrize("tail", [64, 128, 256, 512])
@pytest.mark.parametrize("KVH", [8, 4, 2])
def test_kv8_shared_prefix(tiny, KVH, tail):
    """forks with the share lengths and private lengths of the bf16 test; the shared rows are the source's BF16 rows (its shadow below
    its own boundary is NaN, and so is every fork's shadow below L), the private rows [kv8_from, pos) come from the fork's shadow"""
    model, _ = tiny
    worst = Worst()
    for case in ac.shared_cases(KVH, tail // 4):
        for mode in kc.MODES:
            k8 = kc.Kv8Case(case, mode, tail // 4)
            for gqa in _gqa_values(KVH):
                fam = _tail_family(tail, KVH, gqa) + " KV8"
                for nt, up, sp in _configs(mode):
                    _check8(model, k8, 16, worst, fam + (" + k_attn_prefix_g" if up else ""), "shared", use_prefix=up, pfx_splits=sp, tail=tail,
                            gqa=gqa, nt=nt)
    worst.show(f"attn_decode_b8 shared KVH{KVH} tail {tail}")


def test_kv8_grouping_and_company(tiny):
    """the 64-slot grouping case; a slot alone gives the bits it gave in company; 16, 32 and 64 slots give the same bits"""
    model, _ = tiny
    worst = Worst()
    case = ac.grouping_case()
    kw = dict(use_prefix=1, pfx_splits=4, tail=128, gqa=1, nt=1)
    fam = _tail_family(kw["tail"], case.KVH, kw["gqa"]) + " KV8"
    for mode in ("L", "mid", "pos"):
        k8 = kc.Kv8Case(case, mode, 32)
        out = _check8(model, k8, 64, worst, fam + " + k_attn_prefix_g", "grouping", **kw)
        _check8(model, k8, 64, worst, fam, "grouping", **dict(kw, use_prefix=0))
        for n, only in ((16, 5), (32, 17), (64, 22)):
            alone, _, _ = _run8(model, k8, n, active=[int(s == only) for s in range(n)], **kw)
            assert np.array_equal(alone[only], out[only]) and (np.delete(alone, only, axis=0) == SENTINEL).all(), (mode, n, only)
        first16 = [int(case.active[s] and s < 16) for s in range(64)]
        outs = [_check8(model, k8, n, worst, fam + " + k_attn_prefix_g", "slot count", active=first16, **kw) for n in (16, 32, 64)]
        assert np.array_equal(outs[0], outs[1][:16]) and np.array_equal(outs[0], outs[2][:16]), mode
    worst.show("attn_decode_b8 grouping (64 slots)")


@pytest.mark.parametrize("tail", [512, 1024])
@pytest.mark.parametrize("nslots", [1, 2, 4])
def test_kv8_multi_vector_grid(tiny, nslots, tail):
    """the <= 4-slot step's grid: 512 / 1024 threads with 1, 2 and 4 slots, no prefix kernel"""
    model, _ = tiny
    worst = Worst()
    rows = tail // 4
    for KVH in (8, 2):
        layouts = [[{"pos": 319}, {"pos": rows}, {"pos": 0}, {"pos": min(2 * rows - 1, 319)}][:nslots]]
        if nslots > 1:
            layouts.append([{"pos": 319}, {"pos": min(64 + rows, 319), "src": 0, "L": 64}, {"pos": 3, "src": 0, "L": 3}, {"pos": 255 + 1, "src": 0, "L": 255}][:nslots])
        for i, slots in enumerate(layouts):
            case = ac.BatchCase(KVH, slots, seed=50 * nslots + KVH + i, rows=rows)
            for mode in kc.MODES:
                k8 = kc.Kv8Case(case, mode, rows)
                for gqa in (0, 1):
                    for nt, up, sp in _configs(mode, prefix_ok=False):
                        _check8(model, k8, nslots, worst, _tail_family(tail, KVH, gqa) + " KV8", "multi-vector", use_prefix=up, pfx_splits=sp,
                                tail=tail, gqa=gqa, nt=nt)
    worst.show(f"attn_decode_b8 multi-vector {nslots} slots tail {tail}")


def test_kv8_op_refusals(tiny):
    model, _ = tiny
    case = ac.unshared_case(8, 32)
    k8 = kc.Kv8Case(case, "mid", 32)
    s = case.pos.index(319)
    for bad in (-1, 320):
        k8.frm[s] = bad
        with pytest.raises(Exception, match="kv8_from"):
            _run8(model, k8, 16, use_prefix=0, pfx_splits=1, tail=128, gqa=1, nt=1)
