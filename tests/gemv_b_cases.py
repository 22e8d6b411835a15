"""Inputs and the float64 reference of the batched decode GEMV op tests (tests/test_gemv_b_host.py checks them on the CPU,
tests/test_gpu_gemv_b.py feeds the same objects to dtk_op_gemv_b / dtk_op_gemv_bkp).

A case holds the operands of one role for all 64 slots: every slot has its own random x (a slot swap fails everywhere) and its own
position (POS is a permutation of 0 .. T_MAX - 1, T_MAX = 64: with the 16 .. 32 rows the issue suggests 64 slots could not all differ;
slot 0 sits at T_MAX - 1, slot 2 one below it, slot 1 at 0 — not slot 0, which runs alone at nslots = 1, where sin = 0 would hide a RoPE sign), fp8 rows carry the scales 2^(b + r % 7) — seven binades, neighbours, rows 16 or 64
apart and the gate / up partners all differ, so one row's scale on another row is a factor >= 2 — over e4m3 codes sized so that the
de-quantised rows have one magnitude.  A run is a prefix of the slots (nslots) with some of them idle; what a slot receives does not
depend on the others, so the reference is computed once per case.

Reference: the dot products in float64 over the bf16 operands (fp8: code value x power-of-two scale, exact), rounded to bf16, then the
HF rounding chain with oracle/llama.py's rmsnorm and apply_rope and the oracle's SwiGLU / residual lines.  `mode="f32"` is the same
chain on oracle.ops.linear (float32 accumulation): the second legitimate reference that sets the bar of the chained outputs.

Every result buffer starts as a quiet NaN with a payload of its own (the residual rows of active slots excepted: they are an input);
judge() demands that every cell outside the ones the role writes still holds its bits.

Bars.  Single-rounding outputs (STORE, LOGITS, V rows, the RESID projection = result - residual in float64, the sum of the partial
planes): test_op_gemv's rel-L2 < 1e-3, <= 2.01 bf16 ulps, < 5 % of the elements differing.  Chained outputs (q / k after RoPE,
SwiGLU, the residual after the add, the normalised rows): twice the worst distance between the two references over every case of
this file — every run's tensor, and every slot's rows on their own: a one-slot run is judged on 24 .. 4096 values, where one rounding
flip is a large rel-L2 — capped at test_op_attention's 4.01 ulps / 2e-3.  q / k after RoPE on random operands are measured in ulps of
their (i, i + 64) pair's length (rope_pair_magnitude): in ulps of the element the two references are 4.41 apart (RAW_ROPE_ULPS), beyond
the cap, because x1 c - x2 s can be far smaller than its terms.  Measured (tests/test_gemv_b_host.py asserts them): worst 1.44 ulps (the
normalised rows; SwiGLU 0.71, q / k 0.71, the residual after the add 0.69) and rel-L2 1.03e-3 (q / k of one slot; the normalised rows of
one slot 4.9e-4, the residual 1.9e-4, SwiGLU 4.1e-5) -> the bar is 2.88 ulps and rel-L2 < 2e-3 (the cap).
GRID cases (operands on a grid of eighths: every partial sum is exact in fp32 whatever the order, so the projection has ONE value)
have no legitimate second answer: what they write must equal the reference bit for bit — q / k / v, logits, stored rows and the
residual after the add; only what passes through expf or rsqrt (the SwiGLU activation, the normalised rows) keeps the chained bar.
They hold every QKV shape, every 64-slot shape and the residual add at realistic magnitudes (the SPLIT block map, N = 2048 / 4096) to
equality, and carry the one listed fault that is <= 1 ulp on random operands, `res + p` rounded once instead of twice.  What they cannot
show is a summation ORDER: the 64-slot shapes and two small QKV shapes therefore run on random operands as well, under the bars and —
the GPU test — to bit equality between the kernels that promise k_gemv_b's order.

Unreachable at these shapes (so not exercised): the RESID shapes behind DTK_GB_RESID_WAVES / DTK_GB_RESID_KS (environment only);
3 and 4 units per block of k_gemv_bl / k_gemv_br and 2 / 3 pair units per block of k_gemv_bus (they follow from groups / CU count > 2);
k_gemv_bus's second qkv block map (v0 = 0: block b owns pair unit b AND V row tile b, taken when pair units <= CUs < pair units + V
tiles — the 7B models' path; H/KVH 2/1 and 2/2 give 20 and 32 blocks, so every block owns a pair unit OR a V tile);
gemv_bl bit 3 without bit 4 (needs (H + KVH) * 16 >= 3/4 of the CUs); k_gemv_br at K = 2048 (the launcher admits K = 4096 only)."""
from __future__ import annotations

import numpy as np
import torch

from oracle.llama import apply_rope, rmsnorm, rope_tables
from oracle.ops import bits_to_f32, f32_to_bits, linear, rb
from tests.helpers import rel_l2

STORE, RESID, QKV, SWIGLU, LOGITS, BKP = 0, 1, 2, 3, 4, 5
EPI_NAME = {STORE: "store", RESID: "resid", QKV: "qkv", SWIGLU: "swiglu", LOGITS: "logits", BKP: "bkp"}
SLOTS = 64
T_MAX = 64
EPS = 1e-5
POS = [T_MAX - 1 - s // 2 if s % 2 == 0 else s // 2 for s in range(SLOTS)]
IDLE = (3, 16, 31, 47, 63)
# quiet NaNs, one payload per buffer
NAN_Q, NAN_K, NAN_V, NAN_Y, NAN_FRAG, NAN_XN, NAN_LOGITS = 0x7FC1, 0x7FC2, 0x7FC3, 0x7FC4, 0x7FC5, 0x7FC6, 0x7FC00007

SINGLE_RL2, SINGLE_ULPS, SINGLE_FRAC = 1e-3, 2.01, 0.05                 # test_op_gemv
MEASURED_CHAIN_ULPS, MEASURED_CHAIN_RL2 = 1.44, 1.03e-3                 # float64 vs float32 reference, worst over every case below
RAW_ROPE_ULPS = 4.41        # q / k on random operands, float64 vs float32 reference, in ulps of the element: why they are not measured so
CHAIN_ULPS, CHAIN_RL2 = min(4.01, 2 * MEASURED_CHAIN_ULPS), min(2e-3, 2 * MEASURED_CHAIN_RL2)

MUTATIONS = ("slot_swap", "pos_off", "rope_sign", "gate_up_swap", "drop_kstep", "dup_kstep", "drop_last_partial", "scale_up", "scale_down",
             "resid_once")


def active_sets(nslots):
    """the layouts a case is run with: idle slots inside the column tiles; at 64 slots also a whole idle tile and a single active slot"""
    out = {"interleaved": [0 if s in IDLE and nslots > 1 else 1 for s in range(nslots)]}
    if nslots == SLOTS:
        out["idle_tile"] = [0 if 16 <= s < 32 or s in IDLE else 1 for s in range(SLOTS)]
        out["one_slot"] = [1 if s == 37 else 0 for s in range(SLOTS)]
    return out


def ulp_report(got, ref, mag=None):
    """tests/test_gpu_parity.py::ulp_report on two fp32 tensors: fraction of elements that differ, max difference in bf16 ulps of the
    reference (floored at 1 % of the tensor's largest magnitude), rel-L2.  NaN anywhere in `got` gives NaN figures, which miss every bar.
    mag (q / k after RoPE on random operands): the element is judged on max(|ref|, mag) — see rope_pair_magnitude."""
    got, ref = torch.as_tensor(got, dtype=torch.float32).reshape(-1), rb(torch.as_tensor(ref, dtype=torch.float32)).reshape(-1)
    if got.numel() == 0:
        return 0.0, 0.0, 0.0
    diff = (got - ref).abs()
    ulp = torch.clamp(ref.abs(), min=1e-2 * float(ref.abs().max()) + 1e-30)
    if mag is not None:
        ulp = torch.maximum(ulp, mag.reshape(-1))
    ulp = ulp * 2.0 ** -7
    return float((diff != 0).float().mean()), float((diff / ulp).max()), rel_l2(got, ref)


def rope_pair_magnitude(o):
    """o [64][heads * 128] after RoPE -> the length of each (i, i + 64) pair, at both places of the pair.  o1 = x1 c - x2 s can be far
    smaller than x1 and x2, and one legitimate rounding flip of x1 then is many ulps OF o1 (the float32 oracle itself is 4.4 ulps from
    float64 that way); what a flip can move is bounded in ulps of the pair's length, which the rotation keeps."""
    t = o.reshape(SLOTS, -1, 2, 64)
    return t.pow(2).sum(2, keepdim=True).sqrt().expand_as(t).reshape(SLOTS, -1)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _nan16(shape, bits):
    return np.full(shape, bits, dtype=np.uint16)


class Case:
    def __init__(self, epi, fmt, K, N=0, H=0, KVH=0, ff=0, norm=False, grid=False, seed=0):
        self.epi, self.fmt, self.K, self.norm, self.grid = epi, fmt, K, norm, grid
        self.H, self.KVH, self.ff = H, KVH, ff
        self.N = N if epi in (STORE, RESID, LOGITS, BKP) else ((H + 2 * KVH) * 128 if epi == QKV else 2 * ff)
        self.d = H * 128 if epi == QKV else K
        N = self.N
        g = torch.Generator().manual_seed(1000 * epi + 7 * K + N + (500 if fmt == "fp8" else 0) + seed)
        e = torch.arange(N) % 7
        if grid:
            self.X = torch.randint(-8, 9, (SLOTS, K), generator=g).float() / 8
            q = torch.randint(-8, 9, (N, K), generator=g).float()
            self.wscale = torch.exp2(-3.0 - e) if fmt == "fp8" else torch.full((N,), 0.125)
        else:
            self.X = rb(torch.randn(SLOTS, K, generator=g))
            # codes of magnitude ~ 8 * 2^-(r % 7) under the scale 2^(b + r % 7): de-quantised rows of one magnitude, ~ K^-1/2
            q = (torch.randn(N, K, generator=g) * 8 * torch.exp2(-e.float())[:, None]).to(torch.float8_e4m3fn).float()
            self.wscale = torch.exp2(-3.0 - round(0.5 * float(np.log2(K))) + e)
        if fmt == "fp8":
            self.W8 = q.to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()
            assert torch.equal(torch.from_numpy(self.W8).view(torch.float8_e4m3fn).float(), q)
            self.Wq = q                                  # the code values; W = Wq * wscale[:, None]
        else:
            self.W8 = None
            self.Wq = q if grid else rb(torch.randn(N, K, generator=g) * K ** -0.5 / 0.0625)
            self.wscale = torch.full((N,), 0.125 if grid else 0.0625)       # (bf16: one exact factor, so that W = Wq * wscale in both formats)
        self.W = self.Wq * self.wscale[:, None]
        assert torch.equal(rb(self.W), self.W)
        self.norm_w = rb(1 + 0.1 * torch.randn(N if epi == BKP else K, generator=g))
        self.pos = list(POS)
        self._ref = {}
        if epi in (RESID, BKP):
            if grid:
                self.res = rb(torch.randn(SLOTS, N, generator=g))
            else:
                # The bar of the RESID projection is a single rounding's, and result - residual gives the projection back only if the add
                # rounds nothing away: the residual is -sign(p) * m ulps of the reference projection, m = 1..3, so residual + bf16(p) is a
                # bf16 number for the reference's p and for a p one ulp beside it.  (What the add rounds is the GRID cases' matter.)
                p = rb((self.X_in().double() @ self.W.double().t()).float())
                ulp = torch.exp2(torch.floor(torch.log2(p.abs().clamp(min=2.0 ** -20))) - 7)
                m = torch.randint(1, 4, p.shape, generator=g).float()
                self.res = -torch.sign(p + (p == 0)) * m * ulp
                assert torch.equal(rb(self.res), self.res) and torch.equal(rb(self.res + p), self.res + p)
        if epi == QKV:
            self.cos, self.sin = rope_tables(128, 10000.0, 1.0, T_MAX)

    def X_in(self):
        """the GEMV's input rows: X, or its RMSNorm where the role runs with the norm prologue"""
        return rmsnorm(self.X, self.norm_w, EPS) if (self.norm and self.epi != BKP) else self.X

    @property
    def name(self):
        shape = {QKV: f"H{self.H}KVH{self.KVH}", SWIGLU: f"ff{self.ff}"}.get(self.epi, f"N{self.N}")
        return f"{EPI_NAME[self.epi]}-{shape}-K{self.K}-{self.fmt}" + ("-norm" if self.norm else "") + ("-grid" if self.grid else "")

    # ------------------------------------------------------------------ reference
    def applies(self, m):
        return {"slot_swap": True, "drop_kstep": True, "dup_kstep": True,
                "pos_off": self.epi == QKV, "rope_sign": self.epi == QKV, "gate_up_swap": self.epi == SWIGLU,
                "drop_last_partial": self.K % 32 != 0, "scale_up": self.fmt == "fp8", "scale_down": self.fmt == "fp8",
                "resid_once": self.grid and self.epi in (RESID, BKP)}[m]

    def reference(self, mode="f64", mutate=None):
        """the role's outputs for all 64 slots (fp32 tensors of bf16 values): dict with p (the rounded projection) and, per role, y /
        act / q, k, v / xn; pos = the cache row each slot writes"""
        if mutate is None and mode in self._ref:
            return self._ref[mode]
        xin = self.X_in()
        W, pos = self.W, list(self.pos)
        step = (self.K // 32) // 2          # the k-step the wrong references lose or repeat
        if mutate == "slot_swap":
            xin = xin[[s ^ 1 for s in range(SLOTS)]]
        elif mutate == "drop_kstep":
            xin = xin.clone(); xin[:, step * 32:step * 32 + 32] = 0
        elif mutate == "drop_last_partial":
            xin = xin.clone(); xin[:, self.K // 32 * 32:] = 0
        elif mutate in ("scale_up", "scale_down"):
            W = self.Wq * torch.roll(self.wscale, 1 if mutate == "scale_down" else -1)[:, None]      # row r with the scale of row r -+ 1
        elif mutate == "pos_off":
            pos = [p + 1 if p < T_MAX - 1 else p - 1 for p in pos]
        if mode == "f64":
            acc = xin.double() @ W.double().t()
            if mutate == "dup_kstep":
                acc = acc + xin[:, step * 32:step * 32 + 32].double() @ W[:, step * 32:step * 32 + 32].double().t()
            p = rb(acc.float())
        else:
            assert mutate is None
            acc = None
            p = linear(xin, W)
        out = {"p": p, "pos": pos}
        if self.epi == QKV:
            H, KVH = self.H, self.KVH
            q = p[:, :H * 128].reshape(SLOTS, H, 128).transpose(0, 1)
            k = p[:, H * 128:(H + KVH) * 128].reshape(SLOTS, KVH, 128).transpose(0, 1)
            cos, sin = self.cos[pos], self.sin[pos]
            if mutate == "rope_sign":
                sin = -sin
            out["q"] = apply_rope(q, cos, sin).transpose(0, 1).contiguous()
            out["k"] = apply_rope(k, cos, sin).transpose(0, 1).contiguous()
            out["v"] = p[:, (H + KVH) * 128:].reshape(SLOTS, KVH, 128).contiguous()
        elif self.epi == SWIGLU:
            gate, up = p[:, :self.ff], p[:, self.ff:]
            if mutate == "gate_up_swap":
                gate, up = up, gate
            out["act"] = rb(rb(torch.nn.functional.silu(gate)) * up)
        elif self.epi in (RESID, BKP):
            out["y"] = rb(self.res + (acc.float() if mutate == "resid_once" else p))
            if self.epi == BKP:
                out["xn"] = rmsnorm(out["y"], self.norm_w, EPS)
        if mutate is None:
            self._ref[mode] = out
        return out

    # ------------------------------------------------------------------ buffers
    def initial(self, active):
        """the in/out buffers before the run (numpy bit patterns), all 64 slots"""
        act = np.zeros(SLOTS, dtype=bool); act[:len(active)] = np.asarray(active, dtype=bool)
        if self.epi == QKV:
            kv = (SLOTS, self.KVH, T_MAX, 128)
            return {"q": _nan16((SLOTS, self.H * 128), NAN_Q), "k": _nan16(kv, NAN_K), "v": _nan16(kv, NAN_V)}
        if self.epi == SWIGLU:
            return {"frag": _nan16((4 * ((self.ff + 31) // 32) * 512,), NAN_FRAG), "y": _nan16((SLOTS, self.ff), NAN_Y)}
        if self.epi == LOGITS:
            return {"logits": np.full((SLOTS, self.N), NAN_LOGITS, dtype=np.uint32).view(np.float32)}
        y = _nan16((SLOTS, self.N), NAN_Y)
        if self.epi in (RESID, BKP):
            y[act] = f32_to_bits(self.res)[act]
        return {"y": y, "xn": _nan16((SLOTS, self.N), NAN_XN)} if self.epi == BKP else {"y": y}

    def frag_index(self, nslots):
        """element offsets of (slot, row) in the fragment-major SwiGLU buffer (xtile_off, csrc/common.h)"""
        s, i = np.meshgrid(np.arange(nslots), np.arange(self.ff), indexing="ij")
        nsteps = (self.ff + 31) // 32
        return (((s >> 4) * nsteps + (i >> 5)) * 64 + ((i & 31) >> 3) * 16 + (s & 15)) * 8 + (i & 7)

    def written(self, out, active):
        """what a run that computes `out` leaves in the buffers: initial() with the cells of the active slots filled in"""
        buf = self.initial(active)
        slots = [s for s, a in enumerate(active) if a]
        if self.epi == QKV:
            qb, kb, vb = f32_to_bits(out["q"]), f32_to_bits(out["k"]), f32_to_bits(out["v"])
            for s in slots:
                buf["q"][s] = qb[s].reshape(-1)
                buf["k"][s, :, out["pos"][s]] = kb[s]
                buf["v"][s, :, out["pos"][s]] = vb[s]
        elif self.epi == SWIGLU:
            ab, idx = f32_to_bits(out["act"]), self.frag_index(SLOTS)
            for s in slots:
                buf["frag"][idx[s]] = ab[s]
            buf["y"][:len(active)] = buf["frag"][idx[:len(active)]]        # the op un-tiles the first nslots rows, idle ones included
        elif self.epi == LOGITS:
            buf["logits"][slots] = out["p"].numpy()[slots]
        elif self.epi == STORE:
            buf["y"][slots] = f32_to_bits(out["p"])[slots]
        else:
            buf["y"][slots] = f32_to_bits(out["y"])[slots]
            if self.epi == BKP:
                buf["xn"][slots] = f32_to_bits(out["xn"])[slots]
        return buf

    # ------------------------------------------------------------------ verdict
    def write_mask(self, active):
        """True where a run with this layout writes: the cells in which two runs with different results differ"""
        ref = self.reference()
        a, b = (self.written({k: (torch.full_like(v, c) if torch.is_tensor(v) else v) for k, v in ref.items()}, active) for c in (1.0, 2.0))
        return {n: _bits(a[n]) != _bits(b[n]) for n in a}

    def extract(self, got):
        """the role's outputs as [64][n] fp32 tensors, read from the cells the reference says they are in"""
        ref = self.reference()
        f = lambda bits: bits_to_f32(np.ascontiguousarray(bits))
        every = np.arange(SLOTS)
        if self.epi == QKV:
            return {"q": f(got["q"]), "k": f(got["k"][every, :, ref["pos"]]).reshape(SLOTS, -1), "v": f(got["v"][every, :, ref["pos"]]).reshape(SLOTS, -1)}
        if self.epi == SWIGLU:
            return {"act": f(got["frag"][self.frag_index(SLOTS)])}
        if self.epi == LOGITS:
            return {"p": torch.from_numpy(got["logits"].copy())}
        if self.epi == STORE:
            return {"p": f(got["y"])}
        out = {"y": f(got["y"])}
        if self.epi == BKP:
            out["xn"] = f(got["xn"])
        return out

    def pairs(self, out, partial_sum=None):
        """(single-rounding pairs, chained pairs) of (got, reference) [64][n] tensors"""
        ref = self.reference()
        flat = lambda t: t.reshape(SLOTS, -1)
        if self.epi == QKV:
            rq, rk = flat(ref["q"]), flat(ref["k"])
            if self.grid:
                return [(out["v"], flat(ref["v"]))], [(out["q"], rq), (out["k"], rk)]
            return [(out["v"], flat(ref["v"]))], [(out["q"], rq, rope_pair_magnitude(rq)), (out["k"], rk, rope_pair_magnitude(rk))]
        if self.epi == SWIGLU:
            return [], [(out["act"], ref["act"])]
        if self.epi in (LOGITS, STORE):
            return [(out["p"], ref["p"])], []
        single, chain = [], [(out["y"], ref["y"])]
        if not self.grid:       # the projected part (a GRID residual is as large as the projection: its result is held to equality instead)
            single.append(((out["y"].double() - self.res.double()).float(), ref["p"]))
        if self.epi == BKP:
            chain.append((out["xn"], ref["xn"]))
            if partial_sum is not None:
                single.append((rb(torch.as_tensor(np.asarray(partial_sum), dtype=torch.float32)), ref["p"]))
        return single, chain

    def reference_distance(self):
        """worst (ulps, rel-L2) of the chained outputs between the float32 and the float64 reference, over every run of the case and
        over every slot on its own (the tensors of the one-slot runs, of which the GPU test makes a few)"""
        far = self.reference("f32")
        out = {k: (v.reshape(SLOTS, -1) if torch.is_tensor(v) else v) for k, v in far.items()}
        chain = self.pairs(out)[1]
        wu = wr = 0.0
        for g_, r_, *m_ in chain:
            for _, _, act in runs(self):
                slots = [s for s, a in enumerate(act) if a]
                _, u, r = ulp_report(g_[slots], r_[slots], *(t[slots] for t in m_))
                wu, wr = max(wu, u), max(wr, r)
            ulp = torch.clamp(r_.abs(), min=1e-2 * r_.abs().amax(1, keepdim=True) + 1e-30)
            ulp = (torch.maximum(ulp, m_[0]) if m_ else ulp) * 2.0 ** -7
            d = (g_ - r_).abs()
            wu = max(wu, float((d / ulp).max()))
            wr = max(wr, float((d.double().norm(dim=1) / (r_.double().norm(dim=1) + 1e-30)).max()))
        return wu, wr

    def raw_rope_distance(self):
        """q / k of the float32 against the float64 reference in ulps of the ELEMENT (the measure the chained bar would use): what rules
        that measure out for RoPE outputs on random operands"""
        far = self.reference("f32")
        return max(ulp_report(far[n].reshape(SLOTS, -1), self.reference()[n].reshape(SLOTS, -1))[1] for n in ("q", "k"))

    def judge(self, got, active, partial_sum=None):
        """got = the buffers after the run.  Returns (ok, figures): cells outside the role's own bit-equal to what they held, single-rounding
        outputs and chained outputs under their bars (GRID cases: every written cell equal to the reference's bit for bit, the normalised
        rows excepted — their scale comes from an fp32 sum of squares and an rsqrt)."""
        ref = self.reference()
        want, init, mask = self.written(ref, active), self.initial(active), self.write_mask(active)
        slots = [s for s, a in enumerate(active) if a]
        fig = {"untouched": True, "exact": True, "single": (0.0, 0.0, 0.0), "chain": (0.0, 0.0)}
        for name in want:
            g8, i8, w8 = _bits(got[name]), _bits(init[name]), _bits(want[name])
            if self.epi == SWIGLU and name == "y":      # out only: the first nslots rows of the fragment buffer, row-major
                fig["untouched"] = fig["untouched"] and np.array_equal(got["y"][:len(active)], got["frag"][self.frag_index(len(active))]) \
                    and np.array_equal(got["y"][len(active):], init["y"][len(active):])
                continue
            if not np.array_equal(g8[~mask[name]], i8[~mask[name]]):
                fig["untouched"] = False
            if self.grid and name not in ("xn", "frag") and not np.array_equal(g8[mask[name]], w8[mask[name]]):
                fig["exact"] = False
        single, chain = self.pairs(self.extract(got), partial_sum)
        single = [(g_[slots], r_[slots]) for g_, r_ in single]
        chain = [tuple(t[slots] for t in c_) for c_ in chain]
        worse = lambda x, y: float("nan") if (x != x or y != y) else max(x, y)
        for a, b in single:
            fig["single"] = tuple(worse(x, y) for x, y in zip(fig["single"], ulp_report(a, b)))
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
        _cache[key] = Case(*a, **kw)
    return _cache[key]


SMALL_K = (40, 72, 256, 304)          # K % 32 = 8, 8, 0, 16: waves without a k-step, an odd fp8 step count, a partial last step
SMALL_NSLOTS = (1, 16, 17, 32, 33, 64)
WIDE = (0, 1, 3, 6)


def small_cases():
    """k_gemv_b: five epilogues x K x bf16 / fp8 at ragged N; the RMSNorm prologue on K = 72 and 256 (not for QKV, which is GRID)"""
    out = []
    for K in SMALL_K:
        norm = K in (72, 256)
        for fmt in ("bf16", "fp8"):
            out += [_case(LOGITS, fmt, K, N=77, norm=norm), _case(LOGITS, fmt, K, N=130, norm=norm),
                    _case(RESID, fmt, K, N=144, norm=norm), _case(RESID, fmt, K, N=200, norm=norm),
                    _case(SWIGLU, fmt, K, ff=24, norm=norm), _case(SWIGLU, fmt, K, ff=88, norm=norm),
                    _case(QKV, fmt, K, H=2, KVH=1, grid=True), _case(QKV, fmt, K, H=2, KVH=2, grid=True),
                    _case(STORE, fmt, K, N=77, norm=norm), _case(STORE, fmt, K, N=144, norm=norm)]
    for fmt in ("bf16", "fp8"):        # the SPLIT block map of resid_split (row-tile pairs a multiple of 8) and a shape beside it
        out += [_case(RESID, fmt, 72, N=256), _case(RESID, fmt, 72, N=224), _case(RESID, fmt, 72, N=144, grid=True),
                _case(RESID, fmt, 72, N=256, grid=True)]
    # q / k / v on random operands (with the norm prologue, and at a partial last k-step)
    out += [_case(QKV, "bf16", 256, H=2, KVH=1, norm=True), _case(QKV, "fp8", 304, H=2, KVH=2)]
    return out


def big_cases(K=2048):
    """the 64-slot kernels' shapes: 5 row-tile groups (not a multiple of 2, 3 or 4 units per block) and one aligned shape per role, each
    on GRID operands (equality with float64) and on random ones (the bars; equality between the kernels, which only operands whose sums
    depend on the order can tell apart)"""
    out = []
    for fmt in ("bf16", "fp8"):
        for grid in (True, False):
            out += [_case(QKV, fmt, K, H=2, KVH=1, grid=grid), _case(QKV, fmt, K, H=2, KVH=2, grid=grid),
                    _case(SWIGLU, fmt, K, ff=80, grid=grid), _case(SWIGLU, fmt, K, ff=96, grid=grid),
                    _case(LOGITS, fmt, K, N=160, grid=grid), _case(LOGITS, fmt, K, N=192, grid=grid)]
    return out


BKP_SHAPES = [(N, K) for N in (2048, 4096) for K in (256, 480, 768)]


def bkp_cases():
    out = [_case(BKP, fmt, K, N=N) for N, K in BKP_SHAPES for fmt in ("bf16", "fp8")]
    return out + [_case(BKP, fmt, K, N=N, grid=True) for N, K in ((2048, 256), (2048, 480), (4096, 768)) for fmt in ("bf16", "fp8")]


def runs(case):
    """(nslots, layout name, active flags) of every run of a case"""
    ns = SMALL_NSLOTS if case.K < 2048 and case.epi != BKP else ((33, 64) if case.epi == BKP else (49, 64))
    return [(n, name, act) for n in ns for name, act in active_sets(n).items()]


def all_cases():
    return small_cases() + big_cases(2048) + big_cases(4096) + bkp_cases()
