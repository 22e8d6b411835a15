"""The weight kernel of the multi-vector decode step (contexts with at most 5 slots), k_gemv_mv, op by op on the MI355X
(dtk_op_gemv_mv_role) against the float64 reference of tests/gemv_mv_cases.py: every (prologue, epilogue) the step launches and the two
EPI_STORE pairs, bf16 and fp8 rows, 1 / 2 / 4 slots, every block shape of launch_mv_nb, every active set, with and without a
BatchState, x as rows and in fragment order.  Every result buffer starts as NaN poison and the op's device scratch as 0xFF bytes; what
a role must not write — an idle slot's rows and caches, cache rows other than pos[slot], fragment cells of slots >= nb — has to keep
its bits, and the op itself fails if anything behind the end of a result buffer was written.

Besides the bars, the promises of kernels_decode_mv.hip's header: all four shapes of a role agree bit for bit (a lane's chunk order and
the norm's 256-thread reduction do not depend on the block); shape -1 is the shape mv_default_shape names; a slot's outputs are
bit-identical whether it travels at nb 1, 2 or 4, in whichever slot index, whatever the other slots hold or whether they are active;
and per slot the outputs equal k_gemv's (dtk_op_gemv_role) bit for bit."""
from __future__ import annotations

import numpy as np
import pytest

from oracle.ops import f32_to_bits
from tests import gemv_cases as gc
from tests import gemv_mv_cases as mc
from tests.test_gpu_gemv import Worst, _p, _same
from tests.test_gpu_gemv import _run as _run_single

pytestmark = pytest.mark.gpu

ROLE_ID = lambda r: f"{gc.PRO_NAME[r[0]]}-{gc.EPI_NAME[r[1]]}-{r[2]}"
ERR_ARG = -1
ROLE_NB = [(r, nb) for r in mc.ROLES for nb in mc.NBS]
ROLE_NB_ID = lambda p: f"{ROLE_ID(p[0])}-nb{p[1]}"


@pytest.fixture(scope="module")
def tiny():
    """any context serves the op (it brings its own weights)"""
    from detikzify_amd.model import load
    return load("detikzify-tiny", synthetic=1234)[0]


def _operands(case):
    if not hasattr(case, "dev"):
        f32 = lambda t: np.ascontiguousarray(t.numpy().astype(np.float32))
        o = dict(W=f32_to_bits(case.W) if case.fmt == "bf16" else None, W8=case.W8, ws=f32(case.wscale) if case.fmt == "fp8" else None,
                 nw=f32_to_bits(case.norm_w) if case.pro == gc.RMSNORM else None, cos=None, sin=None)
        if case.epi == gc.QKV:
            o.update(cos=f32_to_bits(case.cos), sin=f32_to_bits(case.sin))
        case.dev = o
    return case.dev


def _call(model, case, shape, d=None, fill=0xFF, **over):
    """one dtk_op_gemv_mv_role call on poisoned buffers; returns (rc, buffers).  `over` replaces arguments by name (the refusals)."""
    o, buf = _operands(case), case.initial()
    a = dict(pro=case.pro, epi=case.epi, nb=case.nb, shape=shape, W=o["W"], W8=o["W8"], ws=o["ws"], N=case.N, K=case.K,
             d=d if d is not None else (case.d if case.epi == gc.QKV else 0), ff=case.ff, H=case.H, KVH=case.KVH, T_max=gc.T_MAX, pos=list(case.pos),
             active=list(case.active), bs_null=int(case.bs_null), x_layout=case.x_layout, nw=o["nw"])
    a.update(over)
    X = a["X"] if "X" in a else case.x_buffer(a["x_layout"])
    pos, act = np.asarray(a["pos"], dtype=np.int32), np.asarray(a["active"], dtype=np.int32)
    g = lambda n: _p(buf.get(n))
    rc = model.lib.dtk_op_gemv_mv_role(model._ctx, a["pro"], a["epi"], a["nb"], a["shape"], _p(a["W"]), _p(a["W8"]), _p(a["ws"]), a["N"], a["K"],
                                       a["d"], a["ff"], a["H"], a["KVH"], a["T_max"], _p(pos), _p(act), a["bs_null"], a["x_layout"], _p(X),
                                       _p(a["nw"]), gc.EPS, _p(o["cos"]), _p(o["sin"]), fill, g("q"), g("k"), g("v"), g("y"), g("logits"))
    return rc, buf


def _run(model, case, shape, d=None, fill=0xFF, **over):
    rc, buf = _call(model, case, shape, d, fill, **over)
    model._check(rc, f"dtk_op_gemv_mv_role {case.name} shape {shape}")
    return buf


def _judged(model, case, shape, worst, group, d=None, **over):
    buf = _run(model, case, shape, d, **over)
    ok, fig = case.judge(buf)
    if fig["single"][0] == fig["single"][0] and fig["chain"][0] == fig["chain"][0]:
        worst.add(group, fig)
    assert ok, f"{case.name} shape {shape} d {d}: {fig}"
    return buf


# ------------------------------------------------------------------------------------------ every role x format x nb x shape
@pytest.mark.parametrize("role_nb", ROLE_NB, ids=ROLE_NB_ID)
def test_every_shape_against_float64(tiny, role_nb):
    """every case of the role under judge() in shapes 0..3 and -1 (GRID cases bit-exact); the four shapes agree bit for bit; -1 is the
    shape the mirror of mv_default_shape names (for (COPY, RESID) as down, d != K, and as o_proj, d == K)"""
    role, nb = role_nb
    pro, epi, fmt = role
    worst = Worst()
    for case in mc.role_cases(*role, nb):
        got = {}
        for shape in mc.SHAPES:
            U, waves, persistent, bpc = mc.shape_of(pro, epi, fmt, nb, mc.launched_shape(shape, epi, nb, case.K, 0))
            group = f"{ROLE_ID(role)} nb {nb} shape {shape} (U {U}, {waves} waves{', persistent' if persistent else ''})" + (" GRID" if case.grid else "")
            got[shape] = _judged(tiny, case, shape, worst, group)
            assert _same(got[shape], got[0]), f"{case.name}: shape {shape} and shape 0 differ in bits"
        for d in ((None,) if epi != gc.RESID else (case.K + 8, case.K)):
            want = mc.launched_shape(-1, epi, nb, case.K, case.d if epi == gc.QKV else (d or 0))
            buf = _judged(tiny, case, -1, worst, f"{ROLE_ID(role)} nb {nb} default" + (" GRID" if case.grid else ""), d=d)
            assert _same(buf, got[want]), f"{case.name}: shape -1 at d {d} is not shape {want}"
    worst.show()


# ------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize("role", mc.ROLES, ids=ROLE_ID)
def test_a_slot_does_not_depend_on_nb_index_or_fellow_travellers(tiny, role):
    """the four slots of an all-active nb-4 case, re-run alone, in pairs (first and second, beside an active and beside an idle slot, with
    and without a BatchState) and four abreast in another order with holes: each slot's own cells hold the same bits every time"""
    pro, epi, fmt = role
    worst = Worst()
    for base in [c for c in mc.role_cases(*role, 4) if all(c.active) and not c.grid][:3]:
        home = _judged(tiny, base, -1, worst, f"{ROLE_ID(role)} independence")
        trips = [([b], (1,), bool(b & 1)) for b in range(4)]
        trips += [([b, b ^ 1], (1, 1), b == 2) for b in range(4)] + [([b ^ 1, b], (0, 1), False) for b in range(4)] + [([b, (b + 2) % 4], (1, 0), False) for b in range(4)]
        trips += [([3, 2, 1, 0], (1, 1, 1, 1), True), ([1, 3, 0, 2], (1, 0, 1, 1), False), ([2, 0, 3, 1], (0, 1, 1, 0), False), ([1, 2, 3, 0], (0, 0, 0, 1), False)]
        for order, active, null in trips:
            trip = base.travelling(order, active, null)
            for shape in ((-1,) if len(order) > 1 else (-1, 3)):
                buf = _judged(tiny, trip, shape, worst, f"{ROLE_ID(role)} independence")
                for j in trip.live():
                    assert _same(trip.slot_view(buf, j), base.slot_view(home, order[j])), \
                        f"{base.name}: slot {order[j]} as slot {j} of {order} (active {active}, shape {shape}) differs in bits from the slot at home"
    worst.show()


# ------------------------------------------------------------------------------------------ rows = fragment order
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_fragment_order_input_equals_rows(tiny, fmt):
    for epi in (gc.RESID, gc.STORE):
        for nb in mc.NBS:
            for case in mc.role_cases(gc.COPY, epi, fmt, nb):
                for shape in (-1, 0, 3):
                    rows, frag = (_run(tiny, case, shape, x_layout=layout) for layout in (0, 1))
                    assert _same(rows, frag), f"{case.name} shape {shape}: x as rows and in fragment order give different bits"
                    assert case.judge(frag)[0], case.name


# ------------------------------------------------------------------------------------------ k_gemv_mv = k_gemv per slot
TWIN = {(gc.COPY, gc.STORE, "bf16"): 0, (gc.RMSNORM, gc.STORE, "bf16"): 0, (gc.COPY, gc.RESID, "bf16"): 1, (gc.COPY, gc.RESID, "fp8"): 0,
        (gc.RMSNORM, gc.QKV, "bf16"): 0, (gc.RMSNORM, gc.QKV, "fp8"): 0, (gc.RMSNORM, gc.SWIGLU, "bf16"): 0, (gc.RMSNORM, gc.SWIGLU, "fp8"): 0,
        (gc.RMSNORM, gc.LOGITS, "bf16"): 0, (gc.RMSNORM, gc.LOGITS, "fp8"): 0}


@pytest.mark.parametrize("role", sorted(TWIN), ids=ROLE_ID)
def test_every_slot_equals_the_single_sequence_kernel(tiny, role):
    """the promise at the top of kernels_decode_mv.hip: per slot the outputs are k_gemv's bit for bit — a KS = 1 variant under PRO_COPY
    (any: they agree among themselves, tests/test_gpu_gemv.py), a 4-wave KS = 1 variant under PRO_RMSNORM (the norm's reduction is that of
    a 256-thread block).  (k_gemv has no fp8 EPI_STORE.)"""
    R, U, waves, bpc, KS = gc.TABLE[role][TWIN[role]]
    assert KS == 1 and (role[0] == gc.COPY or waves == 4)
    for nb in mc.NBS:
        for case in mc.role_cases(*role, nb):
            buf = _run(tiny, case, -1)
            for b in case.live():
                single = _run_single(tiny, case.slots[b], TWIN[role])
                assert _same(case.slot_view(buf, b), single), f"{case.name}: slot {b} differs in bits from k_gemv variant {TWIN[role]} on its operands"


# ------------------------------------------------------------------------------------------ the second trip of a persistent wave
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_persistent_second_trip(tiny, fmt):
    """nb 4 with a hole, K = 64 and more units than CUs x blocks per CU x waves by less than one round: some waves set their rows again,
    load their first stage and prefetch the next chunk's epilogue operands while this chunk's are still to be used; the others stop"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    worst = Worst()
    for pro, epi in mc.PERSISTENT_ROLES:
        for shape in (1, 2, 3):
            case, first = mc.persistent_case(pro, epi, fmt, shape, cus)
            U, waves, persistent, bpc = mc.shape_of(pro, epi, fmt, 4, shape)
            assert persistent and first == cus * bpc * waves and first < case.units < 2 * first, (case.name, cus, first, case.units)
            role = (pro, epi, fmt)
            buf = _judged(tiny, case, shape, worst, f"{ROLE_ID(role)} persistent shape {shape}")
            assert _same(_judged(tiny, case, 0, worst, f"{ROLE_ID(role)} persistent shape 0"), buf), f"{case.name}: shape {shape} and shape 0 differ in bits"
    worst.show()


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_touch_nothing(tiny):
    """everything batch_step_launches_mv would never launch: DTK_ERR_ARG, nothing uploaded or launched, every buffer as it was"""
    full = dict(active=(1, 1, 1, 1))
    qkv = mc._case(gc.RMSNORM, gc.QKV, "bf16", 4, K=72, H=2, KVH=1, **full)
    qkv8 = mc._case(gc.RMSNORM, gc.QKV, "fp8", 4, K=1040, H=2, KVH=1, **full)
    swi = mc._case(gc.RMSNORM, gc.SWIGLU, "bf16", 4, K=72, ff=24, **full)
    res = mc._case(gc.COPY, gc.RESID, "bf16", 4, K=72, N=37, **full)
    resf = mc._case(gc.COPY, gc.RESID, "bf16", 4, K=72, N=37, x_layout=1, active=(1, 0, 1, 1))
    res8 = mc._case(gc.COPY, gc.RESID, "fp8", 4, K=1040, N=37, **full)
    log = mc._case(gc.RMSNORM, gc.LOGITS, "bf16", 4, K=72, N=37, **full)
    sto = mc._case(gc.COPY, gc.STORE, "bf16", 4, K=72, N=37, **full)
    bad = [  # a (prologue, epilogue) outside the step's pairs and the two STORE pairs
           (res, -1, dict(pro=gc.RMSNORM)), (log, -1, dict(pro=gc.COPY)), (swi, -1, dict(pro=gc.COPY)), (qkv, -1, dict(pro=gc.COPY)),
           (res, -1, dict(pro=gc.ATTN)), (res, -1, dict(pro=3)), (res, -1, dict(epi=5)), (res, -1, dict(epi=-1)), (res, -1, dict(pro=-1)),
           # nb, shape
           (res, -1, dict(nb=0)), (res, -1, dict(nb=3)), (res, -1, dict(nb=5)), (res, -1, dict(nb=8)), (res, 4, {}), (res, -2, {}), (qkv, 4, {}),
           # K
           (res, -1, dict(K=76)), (res, -1, dict(K=0)), (res8, -1, dict(K=1032)), (res, -1, dict(W=None)),
           (res, -1, dict(W8=res8.W8, ws=np.ones(37, dtype=np.float32))), (res8, -1, dict(ws=None)),
           # QKV
           (qkv, -1, dict(N=qkv.N - 128)), (qkv, -1, dict(d=qkv.d + 128)), (qkv, -1, dict(KVH=2)), (qkv, -1, dict(H=3, KVH=2, N=7 * 128, d=3 * 128)),
           (qkv, -1, dict(pos=[7, 3, -1, 1])), (qkv, -1, dict(pos=[7, 3, 5, gc.T_MAX])), (qkv8, -1, dict(pos=[gc.T_MAX, 3, 5, 1])),
           # SWIGLU
           (swi, -1, dict(ff=20, N=40)), (swi, -1, dict(N=40)), (swi, -1, dict(ff=0, N=0)),
           # the input layout, the BatchState, the LDS request
           (log, -1, dict(x_layout=1)), (qkv, -1, dict(x_layout=1)), (res, -1, dict(x_layout=2)),
           (res, -1, dict(bs_null=1, active=[1, 0, 1, 1])), (resf, -1, dict(bs_null=1)),
           (res, -1, dict(K=20480)), (res, 3, dict(K=20472))]
    for case, shape, over in bad:
        rc, buf = _call(tiny, case, shape, **over)
        init = case.initial()
        assert rc == ERR_ARG, (case.name, shape, over.keys(), rc)
        assert all(np.array_equal(buf[n].view(np.uint8), init[n].view(np.uint8)) for n in init), (case.name, shape, list(over))
    # (and the same calls without the fault are taken)
    for case in (qkv, qkv8, swi, res, resf, res8, log, sto):
        assert case.judge(_run(tiny, case, -1))[0], case.name
