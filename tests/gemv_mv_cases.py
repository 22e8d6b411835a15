"""Inputs and the float64 reference of the multi-vector decode GEMV op tests (tests/test_gemv_mv_host.py checks them on the CPU,
tests/test_gpu_gemv_mv.py feeds the same objects to dtk_op_gemv_mv_role).

A case holds the operands of ONE role of k_gemv_mv (csrc/kernels_decode_mv.hip) — (RMSNORM, QKV), (COPY, RESID), (RMSNORM, SWIGLU),
(RMSNORM, LOGITS) and the tests' own (COPY, STORE), (RMSNORM, STORE) — in one weight format (bf16; fp8 = e4m3 codes x a per-row
power-of-two scale: the family has no MXFP4 or 13-bit kernels), for nb = 1 | 2 | 4 slots of which `active` decode, with or without a
BatchState (bs_null) and, under PRO_COPY, with x as rows or in fragment order (x_layout 1: common.h's xtile_off).  It is run once per
block shape -1..3; shape_of() below mirrors launch_mv_nb as shape -> (U, waves, persistent, blocks per CU) with the fp8 rule "U halved,
16 waves -> 8", default_shape() mirrors mv_default_shape.  Head dim 128 throughout (the step has no other).

Per slot a case is a tests/gemv_cases.Case: one W, norm_w and wscale (slot 0's) shared by all slots, x, residual and pos per slot.  The
reference is that class's chain slot by slot (float64 dots over the exact operands rounded to bf16, oracle/llama.py's roundings;
mode="f32" = the same chain on oracle.ops.linear, the second legitimate reference), GRID operands follow its rules and give bit-exact
results (SwiGLU excepted).  Positions are pairwise different, never 0 and include T_MAX - 1; idle slots have operands too (the kernel
stages every slot's x), only no result.

Every buffer starts as a quiet NaN with a payload of its own (the residual rows excepted: inputs, idle slots' included); judge() demands
that every cell outside write_mask() keeps its bits: idle slots' rows of q / logits / y and their whole caches, every cache row other
than pos[slot], the fragment cells of slots >= nb and of k >= ff.  The fragment-order input carries poison in the cells of slots >= nb.

Bars.  Single-rounding outputs: gemv_cases.SINGLE_*.  Chained outputs: twice the worst distance between the two references over every
case of this file, its persistent cases and further operand draws of its small ones (redraws()), capped at test_op_attention's 4.01
ulps / 2e-3.  Measured (tests/test_gemv_mv_host.py asserts the figures): 3.92 ulps and rel-L2 1.89e-3, both on the 4 x 37 logits of
K = 4104 (one flip of a normalised x beside a logit near zero, where the 1 % floor of ulp_report counts it as several ulps): twice
that is beyond the caps, so the bar IS the caps.  The single-sequence figures of gemv_cases are not used: the case list differs."""
from __future__ import annotations

import copy

import numpy as np
import torch

from oracle.ops import bits_to_f32, f32_to_bits, rb
from tests import gemv_cases as gc
from tests.gemv_b_cases import ulp_report
from tests.gemv_cases import COPY, EPI_NAME, EPS, LOGITS, NAN_K, NAN_LOGITS, NAN_Q, NAN_V, NAN_Y, PRO_NAME, QKV, RESID, RMSNORM, STORE, SWIGLU, T_MAX  # noqa: F401

NAN_X = 0x7FC5                              # the fragment-order input's cells of slots >= nb and of k >= K
POS = (T_MAX - 1, 3, 5, 1)                  # slot -> position
SINGLE_RL2, SINGLE_ULPS, SINGLE_FRAC = gc.SINGLE_RL2, gc.SINGLE_ULPS, gc.SINGLE_FRAC
MEASURED_CHAIN_ULPS, MEASURED_CHAIN_RL2 = 3.92, 1.89e-3      # float64 vs float32 reference, worst over every case below and its redraws
CHAIN_ULPS, CHAIN_RL2 = min(4.01, 2 * MEASURED_CHAIN_ULPS), min(2e-3, 2 * MEASURED_CHAIN_RL2)

ROLES = [(pro, epi, fmt) for fmt in ("bf16", "fp8") for pro, epi in ((COPY, STORE), (RMSNORM, STORE), (COPY, RESID), (RMSNORM, QKV), (RMSNORM, SWIGLU),
                                                                     (RMSNORM, LOGITS))]
NBS = (1, 2, 4)
SHAPES = (0, 1, 2, 3)
MV_MUTATIONS = ("slot_swap", "x_of_slot0", "pos_of_other_slot", "kv_stride_zero", "idle_slot_written", "frag_piece_transposed", "resid_of_other_slot")
SLOT_MUTATIONS = ("rope_sign", "rope_partner_scale", "gate_up_swap", "kv_section_shift", "drop_kgroup", "dup_kgroup", "drop_tail_chunk", "scale_up",
                  "scale_down", "resid_once")
MUTATIONS = MV_MUTATIONS + SLOT_MUTATIONS
LDS_CU = 160 * 1024


# ---------------------------------------------------------------------------------------------------- the launcher's tables
def shape_of(pro, epi, fmt, nb, shape):
    """launch_mv_nb: (U, waves, persistent, blocks per CU) of block shape 0..3 (R = 1 everywhere)"""
    ur = 8 if nb == 1 else 4
    if (pro, epi) in ((RMSNORM, QKV), (RMSNORM, SWIGLU)):
        t = {0: (2, 4, False, 0), 1: (2, 8, True, 2), 2: (2, 4, True, 4), 3: (2, 16, True, 1)}
    elif (pro, epi) == (RMSNORM, LOGITS):
        t = {0: (4, 4, False, 0), 1: (4, 8, True, 2), 2: (4, 4, True, 4), 3: (2, 16, True, 1)}
    elif (pro, epi) == (COPY, RESID):
        t = {0: (ur, 8, False, 0), 1: (ur, 8, True, 2), 2: (ur, 4, True, 4), 3: (4, 16, True, 1)}
    else:
        assert epi == STORE and pro in (COPY, RMSNORM)
        t = {s: (2, 4, False, 0) for s in SHAPES}
    U, waves, persistent, bpc = t[shape]
    if fmt == "fp8":              # 16 weights per chunk: half the chunks per stage; the one-block-per-CU shape runs 8 waves
        U, waves = (U // 2 if U >= 2 else 1), (8 if waves == 16 else waves)
    return U, waves, persistent, bpc


def default_shape(epi, nb, K, d):
    """mv_default_shape"""
    if nb <= 1:
        return 0
    if nb * K * 2 > 64 * 1024:
        return 3
    if nb == 2:
        return 3 if (epi == RESID and K != d) else 0
    return 1 if epi == QKV else 3


def launched_shape(shape, epi, nb, K, d):
    """launch_gemv_mv: the shape that runs (more than 64 KiB of x forces the one-block-per-CU shape)"""
    s = default_shape(epi, nb, K, d) if shape < 0 else shape
    return 3 if nb * K * 2 > 64 * 1024 else s


def lds_bytes(nb, K, waves):
    """launch_mv_t's dynamic LDS request"""
    return nb * (K >> 3) * 16 + nb * waves * 4 + 64


# ---------------------------------------------------------------------------------------------------- fragment order
def frag_elems(n):
    """whole 16-slot tiles over n values per slot"""
    return (n + 31) // 32 * 512


def frag_off(slot, k):
    """xtile_off (common.h) for slots < 16"""
    k = np.asarray(k)
    return (((k >> 5) * 64 + ((k & 31) >> 3) * 16 + slot) * 8 + (k & 7)).astype(np.int64)


def frag_off_transposed(slot, k):
    """the wrong order: the 8-k piece and the slot swapped"""
    k = np.asarray(k)
    return (((k >> 5) * 64 + slot * 16 + ((k & 31) >> 3)) * 8 + (k & 7)).astype(np.int64)


def to_frag(rows, poison=NAN_X):
    """rows [nb][n] uint16 -> the fragment-order buffer; every other cell holds the poison"""
    nb, n = rows.shape
    out = np.full(frag_elems(n), poison, dtype=np.uint16)
    for b in range(nb):
        out[frag_off(b, np.arange(n))] = rows[b]
    return out


def from_frag(frag, slot, n, off=frag_off):
    return frag[off(slot, np.arange(n))]


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


class MvCase:
    def __init__(self, pro, epi, fmt, nb, active, K=0, N=0, H=0, KVH=0, ff=0, grid=False, bs_null=False, x_layout=0, seed=0, tag=""):
        assert len(active) == nb and nb in NBS and any(active) and not (bs_null and not all(active)) and not (x_layout and pro != COPY)
        self.pro, self.epi, self.fmt, self.nb, self.active, self.grid = pro, epi, fmt, nb, tuple(int(a) for a in active), grid
        self.bs_null, self.x_layout, self.tag, self.seed = bool(bs_null), x_layout, tag, seed
        self.slots = [gc.Case(pro, epi, fmt, K, N=N, H=H, KVH=KVH, hd=128, ff=ff, grid=grid, pos=POS[b], seed=seed + 101 * b) for b in range(nb)]
        s0 = self.slots[0]
        self.K, self.N, self.H, self.KVH, self.ff, self.d, self.units = s0.K, s0.N, H, KVH, ff, s0.d, s0.units
        self.W, self.W8, self.wscale, self.norm_w = s0.W, s0.W8, s0.wscale, s0.norm_w
        self.pos = [s.pos for s in self.slots]
        g = torch.Generator().manual_seed(77003 + 13 * K + 7 * s0.N + nb + seed)
        for s in self.slots[1:]:
            s.W, s.W8, s.wscale, s.norm_w = s0.W, s0.W8, s0.wscale, s0.norm_w
            if fmt == "fp8":
                s.Wq = s0.Wq
            if epi == RESID and not grid:       # gemv_cases' residual (a few ulps of the projection, so that the add rounds nothing away) for the shared W
                p = rb((s.x_in().double() @ s.W.double().t()).float())
                ulp = torch.exp2(torch.floor(torch.log2(p.abs().clamp(min=2.0 ** -20))) - 7)
                s.res = -torch.sign(p + (p == 0)) * torch.randint(1, 4, p.shape, generator=g).float() * ulp
                assert torch.equal(rb(s.res), s.res) and torch.equal(rb(s.res + p), s.res + p)
            s._ref = {}
        if epi == QKV:
            self.cos, self.sin = s0.cos, s0.sin
        assert len(set(self.pos)) == nb and 0 not in self.pos and T_MAX - 1 in self.pos

    def travelling(self, order, active, bs_null=False):
        """this case's slots order[0], order[1], .. (operands, residual and position each) as the slots 0, 1, .. of a step of len(order)
        vectors: what the independence test re-runs them as"""
        new = copy.copy(self)
        new.slots, new.nb, new.active, new.bs_null = [self.slots[i] for i in order], len(order), tuple(int(a) for a in active), bool(bs_null)
        new.pos = [s.pos for s in new.slots]
        new.tag = self.tag + "-as" + "".join(str(i) for i in order)
        assert new.nb in NBS and len(active) == new.nb and len(set(order)) == new.nb and not (bs_null and not all(active))
        if hasattr(new, "ctor"):
            del new.ctor
        return new

    @property
    def name(self):
        shape = {QKV: f"H{self.H}KVH{self.KVH}", SWIGLU: f"ff{self.ff}"}.get(self.epi, f"N{self.N}")
        act = "".join(str(a) for a in self.active)
        return (f"{PRO_NAME[self.pro]}-{EPI_NAME[self.epi]}-{shape}-K{self.K}-{self.fmt}-nb{self.nb}-act{act}" + ("-nobs" if self.bs_null else "") +
                ("-frag" if self.x_layout else "") + ("-grid" if self.grid else "") + self.tag)

    @property
    def chained(self):
        return self.pro != COPY

    def live(self):
        return [b for b in range(self.nb) if self.active[b]]

    def x_rows(self):
        return np.stack([f32_to_bits(s.x) for s in self.slots])

    def x_buffer(self, layout=None):
        """X as it crosses the ABI"""
        return to_frag(self.x_rows()) if (self.x_layout if layout is None else layout) else self.x_rows()

    # ------------------------------------------------------------------ reference
    def pieces_in(self):
        return min(4, self.K // 8)

    def applies(self, m):
        live, nb = self.live(), self.nb
        if m in SLOT_MUTATIONS:
            return self.slots[0].applies(m)
        pieces = {1: self.pieces_in(), 0: 0}[self.x_layout] if self.epi != SWIGLU else min(4, self.ff // 8)
        return {"slot_swap": nb >= 2, "x_of_slot0": any(b > 0 for b in live), "pos_of_other_slot": self.epi == QKV and len(live) >= 2,
                "kv_stride_zero": self.epi == QKV and any(b > 0 for b in live), "idle_slot_written": len(live) < nb,
                # (slot b, piece p) <-> (slot p, piece b): the identity for slot 0 with a single piece
                "frag_piece_transposed": (self.x_layout == 1 or self.epi == SWIGLU) and any(b > 0 or pieces > 1 for b in live),
                "resid_of_other_slot": self.epi == RESID and nb >= 2}[m]

    def outs(self, mode="f64", mutate=None):
        """per slot the role's outputs (gemv_cases.Case.reference), None for an idle slot"""
        live, nb = self.live(), self.nb
        res = [None] * nb
        for b in range(nb):
            if not self.active[b] and mutate != "idle_slot_written":
                continue
            s = self.slots[b]
            if mutate in SLOT_MUTATIONS:
                res[b] = s.reference(mode, mutate)
                continue
            if mutate is not None:
                s = copy.copy(s)
                s._ref = {}
                if mutate == "slot_swap":
                    s.x = self.slots[b ^ 1].x
                elif mutate == "x_of_slot0":
                    s.x = self.slots[0].x
                elif mutate == "pos_of_other_slot":
                    s.pos = self.slots[live[(live.index(b) + 1) % len(live)]].pos
                elif mutate == "resid_of_other_slot":
                    s.res = self.slots[(b + 1) % nb].res
                elif mutate == "frag_piece_transposed" and self.x_layout == 1:
                    s.x = bits_to_f32(from_frag(self.x_buffer(), b, self.K, frag_off_transposed))
            res[b] = s.reference(mode)
        return res

    # ------------------------------------------------------------------ buffers
    def initial(self):
        nb = self.nb
        if self.epi == QKV:
            kv = (nb, self.KVH, T_MAX, 128)
            return {"q": np.full((nb, self.d), NAN_Q, dtype=np.uint16), "k": np.full(kv, NAN_K, dtype=np.uint16), "v": np.full(kv, NAN_V, dtype=np.uint16)}
        if self.epi == LOGITS:
            return {"logits": np.full((nb, self.N), NAN_LOGITS, dtype=np.uint32).view(np.float32)}
        if self.epi == RESID:
            return {"y": np.stack([f32_to_bits(s.res) for s in self.slots])}
        if self.epi == SWIGLU:
            return {"y": np.full(frag_elems(self.ff), NAN_Y, dtype=np.uint16)}
        return {"y": np.full((nb, self.N), NAN_Y, dtype=np.uint16)}

    def written(self, outs, mutate=None):
        """what a run that computes `outs` leaves in the buffers"""
        buf = self.initial()
        for b, out in enumerate(outs):
            if out is None:
                continue
            if self.epi == QKV:
                c = 0 if mutate == "kv_stride_zero" else b
                buf["q"][b] = f32_to_bits(out["q"]).reshape(-1)
                buf["k"][c, :out["k"].shape[0], out["pos"]] = f32_to_bits(out["k"])
                buf["v"][c, :, out["pos"]] = f32_to_bits(out["v"])
            elif self.epi == LOGITS:
                buf["logits"][b] = out["p"].numpy()
            elif self.epi == SWIGLU:
                off = frag_off_transposed if mutate == "frag_piece_transposed" else frag_off
                buf["y"][off(b, np.arange(self.ff))] = f32_to_bits(out["act"])
            else:
                buf["y"][b] = f32_to_bits(out[{RESID: "y", STORE: "p"}[self.epi]])
        return buf

    def write_mask(self):
        ref = self.outs()
        a, b = (self.written([None if o is None else {k: (torch.full_like(v, c) if torch.is_tensor(v) else v) for k, v in o.items()} for o in ref])
                for c in (1.0, 2.0))
        return {n: _bits(a[n]) != _bits(b[n]) for n in a}

    def slot_view(self, got, b):
        """slot b's part of the buffers, shaped as gemv_cases.Case's own"""
        if self.epi == SWIGLU:
            return {"y": from_frag(got["y"], b, self.ff)}
        return {n: a[b] for n, a in got.items()}

    def reference_distance(self):
        wu = wr = 0.0
        for b in self.live():
            u, r = self.slots[b].reference_distance()
            wu, wr = max(wu, u), max(wr, r)
        return wu, wr

    def judge(self, got):
        """got = the buffers after the run.  Returns (ok, figures) as gemv_cases.Case.judge does, the figures the worst over the live slots"""
        ref = self.outs()
        want, init, mask = self.written(ref), self.initial(), self.write_mask()
        fig = {"untouched": True, "exact": True, "single": (0.0, 0.0, 0.0), "chain": (0.0, 0.0)}
        for name in want:
            g8, i8, w8 = _bits(got[name]), _bits(init[name]), _bits(want[name])
            if not np.array_equal(g8[~mask[name]], i8[~mask[name]]):
                fig["untouched"] = False
            if self.grid and self.epi != SWIGLU and not np.array_equal(g8[mask[name]], w8[mask[name]]):
                fig["exact"] = False
        worse = lambda x, y: float("nan") if (x != x or y != y) else max(x, y)
        for b in self.live():
            s = self.slots[b]
            single, chain = s.pairs(s.extract(self.slot_view(got, b)))
            for p, r in single:
                fig["single"] = tuple(worse(x, y) for x, y in zip(fig["single"], ulp_report(p, r)))
            for c_ in chain:
                fig["chain"] = tuple(worse(x, y) for x, y in zip(fig["chain"], ulp_report(*c_)[1:]))
        fr, u, r = fig["single"]
        cu, cr = fig["chain"]
        ok = fig["untouched"] and fig["exact"] and fr < SINGLE_FRAC and u <= SINGLE_ULPS and r < SINGLE_RL2 and cu <= CHAIN_ULPS and cr < CHAIN_RL2
        return bool(ok), fig


# ---------------------------------------------------------------------------------------------------- the case lists
_cache = {}


def _case(*a, **kw):
    key = (a, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = MvCase(*a, **kw)
        _cache[key].ctor = (a, kw)
    return _cache[key]


DISTANCE_DRAWS, DISTANCE_DRAWS_SMALL = 10, 40


def redraws(case):
    """the case on other operand draws: not run anywhere, they only widen the sample the distance between the two references is taken
    over (gemv_cases.redraws).  Two legitimate orders differ by a rounding flip about once in 10^4 outputs; the cases of at most 37 units,
    where one flip weighs most, are too few outputs at ten draws to contain one (ten draws of everything: 0.92 ulps, 1.9e-4), so they are
    drawn forty times."""
    if not case.chained or case.grid or case.N * case.K > 5e5 or not hasattr(case, "ctor"):
        return []
    a, kw = case.ctor
    return [MvCase(*a, **{**kw, "seed": kw.get("seed", 0) + 1000 * s}) for s in range(1, DISTANCE_DRAWS_SMALL if case.units <= 37 else DISTANCE_DRAWS)]


# K: one ragged chunk; 1 / 2 / >= 3 k-groups at every U of shape_of() (test_gemv_mv_host.py computes it); both sides of the norm's
# K8 <= 512 (4096 | 4104, fp8 4112).  (COPY, RESID) besides: the third group of U = 8 at nb 1 (8200; fp8 U = 4: 8208); at nb 4 the LDS
# attribute with the shape not forced (8192: exactly 64 KiB of x), the forced shape 3 (8200; fp8 rows need K % 16: 8208), 11008 and the
# largest request a product model makes (14336: 112 KiB)
K_OF = {"bf16": (8, 72, 1032, 2048, 4096, 4104), "fp8": (16, 1040, 2048, 4096, 4112)}
K_RESID_NB1 = {"bf16": (8200,), "fp8": (8208,)}
K_RESID_NB4 = {"bf16": (8192, 8200, 11008, 14336), "fp8": (8192, 8208, 11008, 14336)}
GRID_K = {"bf16": (72, 2056), "fp8": (1040, 4112)}
N_TAILS = gc.N_TAILS
FF = gc.FF
HEADS = gc.HEADS
# (active, bs_null): every active set of the issue, all-active also without a BatchState
ACTIVE = {1: (((1,), False), ((1,), True)),
          2: (((1, 1), False), ((1, 0), False), ((0, 1), False), ((1, 1), True)),
          4: (((1, 1, 1, 1), False), ((1, 0, 1, 1), False), ((0, 1, 1, 0), False), ((0, 0, 0, 1), False), ((1, 1, 1, 1), True))}


def _vary(nb, i):
    act, null = ACTIVE[nb][i % len(ACTIVE[nb])]
    return dict(active=act, bs_null=null)


def role_ks(pro, epi, fmt, nb):
    ks = K_OF[fmt]
    if (pro, epi) == (COPY, RESID):
        ks = ks + {1: K_RESID_NB1[fmt], 2: (), 4: K_RESID_NB4[fmt]}[nb]
    return ks


def proj_cases(pro, epi, fmt, nb):
    """STORE / RESID / LOGITS over the K list x two of the four N tails per K (gemv_cases._tails); the active sets and, under PRO_COPY, the
    two input layouts in turn; GRID operands on the larger tails"""
    out, n = [], 0
    for i, K in enumerate(role_ks(pro, epi, fmt, nb)):
        for j, N in enumerate(gc._tails(i, K)):
            out.append(_case(pro, epi, fmt, nb, K=K, N=N, x_layout=(i + j) % 2 if pro == COPY else 0, **_vary(nb, n)))
            n += 1
    for i, (K, N) in enumerate(zip(GRID_K[fmt], (130, 257))):
        out.append(_case(pro, epi, fmt, nb, K=K, N=N, grid=True, x_layout=i % 2 if pro == COPY else 0, **_vary(nb, n + i + 1)))
    return out


def swiglu_cases(fmt, nb):
    out, n = [], 0
    for i, K in enumerate(K_OF[fmt]):
        for ff in (FF[i % 3], FF[(i + 1) % 3]):
            out.append(_case(RMSNORM, SWIGLU, fmt, nb, K=K, ff=ff, **_vary(nb, n)))
            n += 1
    return out + [_case(RMSNORM, SWIGLU, fmt, nb, K=K, ff=88, grid=True, **_vary(nb, n + i + 1)) for i, K in enumerate(GRID_K[fmt])]


def qkv_cases(fmt, nb):
    """all three (H, KVH) at the two smallest K, one in turn above"""
    out, n = [], 0
    for i, K in enumerate(K_OF[fmt]):
        for h, kvh in (HEADS if i < 2 else (HEADS[i % 3],)):
            out.append(_case(RMSNORM, QKV, fmt, nb, K=K, H=h, KVH=kvh, **_vary(nb, n)))
            n += 1
    for i, K in enumerate(GRID_K[fmt]):
        out.append(_case(RMSNORM, QKV, fmt, nb, K=K, H=HEADS[i + 1][0], KVH=HEADS[i + 1][1], grid=True, **_vary(nb, n + i + 1)))
    return out


def role_cases(pro, epi, fmt, nb):
    if epi == QKV:
        return qkv_cases(fmt, nb)
    if epi == SWIGLU:
        return swiglu_cases(fmt, nb)
    return proj_cases(pro, epi, fmt, nb)


def all_cases():
    return [c for r in ROLES for nb in NBS for c in role_cases(*r, nb)]


# ---------------------------------------------------------------------------------------------------- the persistent second trip
NOMINAL_CUS = gc.NOMINAL_CUS
PERSISTENT_ROLES = ((COPY, RESID), (RMSNORM, QKV), (RMSNORM, SWIGLU), (RMSNORM, LOGITS))
PERSISTENT_ACTIVE = (1, 0, 1, 1)


def persistent_case(pro, epi, fmt, shape, cus):
    """nb 4 with a hole in the active set, K = 64 and a unit count that exceeds the grid's first round (CUs x blocks per CU x waves) by a
    ragged remainder: some waves take a second chunk — set their rows again, load their first stage and prefetch the next chunk's epilogue
    operands while this chunk's are still pending — the others do not.  Returns (case, first_round_units)."""
    U, waves, persistent, bpc = shape_of(pro, epi, fmt, 4, shape)
    assert persistent
    first = cus * bpc * waves
    kw = dict(K=64, active=PERSISTENT_ACTIVE, tag=f"-persist{shape}")
    if epi == QKV:                       # H + 2 heads of 64 units
        case = _case(pro, epi, fmt, 4, H=-(-first // 64) - 1, KVH=1, **kw)
    elif epi == SWIGLU:
        ff = (first + 40 + 7) // 8 * 8
        ff += 8 * (ff % 7 == 0)          # (gate and up rows ff apart carry different fp8 scales)
        case = _case(pro, epi, fmt, 4, ff=ff, **kw)
    else:
        case = _case(pro, epi, fmt, 4, N=first + 37, x_layout=1 if pro == COPY else 0, **kw)
    return case, first


def persistent_cases(cus=NOMINAL_CUS):
    return [persistent_case(pro, epi, fmt, shape, cus) + (shape,) for fmt in ("bf16", "fp8") for pro, epi in PERSISTENT_ROLES for shape in (1, 2, 3)]
