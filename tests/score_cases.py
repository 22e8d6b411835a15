"""Inputs, references, mirrored maps and mutants of the scoring-head op tests (tests/test_score_op_host.py checks them on the CPU,
tests/test_gpu_score_op.py feeds the same objects to dtk_op_score / dtk_op_score_top).

The kernels under test (csrc/kernels_batched.hip): the log-softmax epilogue of k_gemm_mfma<64, 128, .., LS> and of k_gemm_g3<.., LS> (256 x
128 "tall", 128 x 256 "wide"), which leave one record {m, l, z[target], argmax} per row and 128-column tile; k_score_merge, which folds a
row's records; k_score_top, which computes the picked tiles again and extracts the k best.

Exact logits by construction.  Every class but "random" has operands whose fp32 dot products are exact in ANY k order (the host test
evaluates two), so z = rb(float64 dot) is the one legitimate logit and argmax, zmax, top_ids, top_z and z[target] are judged by equality
of bits against a reference no kernel produced.  Only lse has a bar: the 2e-5 of test_op_score_against_the_gemm_kernels_own_logits,
against logsumexp in float64; logprob and top_logprob are the kernels' own ONE fp32 subtraction of the device's lse from an exact z, so
they are judged by equality of bits too (a target at -1000 needs no tolerance).

Operand classes (channel classes: A[m] has a 1 in base channel b(m) in {0, 1} and a 1 in pattern channel 2 + c(m); W[n][b] = LO[b],
W[n][2 + c] = the pattern's value at column n; so z[m][n] = LO[b] + pattern_c[n], a sum of two bf16 numbers that is a bf16 number):
  lit     pattern = 20 at the lit columns start, start + 67, start + 134, .. (a 64-column half holds at most one), else 0: z is hi = 8
          or lo = -12 (base 1: -4 / -24, the negative maxima at which a record's z[target] starting at 0 shows).  With h lit columns lse
          = hi + log(h + (N - h) e^-20): a lit column lost or counted twice moves lse by >= log(h / (h - 1)) >= 4e-3 (h <= 247).
          The starts move with the row so that every column position of a tile is the only lit column of its half, the argmax and
          the target somewhere (computed by the host test from the mirrored maps below).
  flat    base channel only: every column equal, lse = z0 + log N, at N = 129, 130, 255, 257, 1000 where one column more or less is
          >= 1e-3.
  spread  lit rows whose tiles sit 8 d lower per step d = g |t - T| <= 124 away from the tile T that holds the maximum (first, middle
          and last tile): lit columns 8 - 8 d, the others -12 - 8 d, down to -1004 (base 1: -1016); from d = 13 on exp(m_t - max)
          is 0 in fp32: the far tiles must fold to exactly 0 mass, never to NaN.
  ties    explicit sets of equal maxima: neighbouring lanes, the registers of one lane, the two halves of a tile, different tiles,
          tiles t and t + 64 (the same lane of k_score_merge on different trips), nine in one tile, nine in nine tiles, six in a row
          of the lit spacing.  Argmax is the lowest column; the top-k order is (z descending, id ascending) and the k-th and
          (k + 1)-th entries are equal (where the set is smaller than k, the unlit columns of ALL tiles tie for the rest).
  grid    dense small integers, |a| <= 4, W = integers |w| <= 4 times 2^-6: every partial sum is a multiple of 2^-6 below 2^24 steps,
          exact in any order, and a real k chain runs (K tails included); z = rb(dot) has many exact ties.  The class that checks
          k_score_top's recomputation against the records (top_z[:, 0] == zmax, top_ids[:, 0] == argmax).
  random  normal operands as in test_op_score; the ONLY class that takes its logits from the device's own dtk_op_gemm (set_logits),
          because its fp32 sums have no single value.  On the host its z is rb(float64 dot), a stand-in.

chain() is the second reference: a numpy float32 evaluation of the documented chain (per 64-column half m and sum exp(z - m) in the
lane's order and the wave's butterfly, the half merge, k_score_merge's order: lane q adds tiles q, q + 64, .. ascending, then the
64-lane butterfly).  Its worst distance from the float64 reference is MEASURED_F32_LSE.  The mutants are chain() with one fault."""
from __future__ import annotations

import numpy as np
import torch

from tests.prefill_rows_cases import r64

WT = 512                                    # include/dtk.h: DTK_GEMM_WT
CUS = 256                                   # MI355X
LSE_BAR = 2e-5                              # test_op_score_against_the_gemm_kernels_own_logits
LO = (-12.0, -24.0)                         # base channels 0 / 1
LIT = 20.0                                  # hi = lo + 20 = 8 / -4
SPACING = 67                                # of lit columns: > 64, coprime to 128 and 256
KS = (0, 1, 5, 8)
INT_MAX = 0x7FFFFFFF

# worst |lse(chain, float32) - lse(float64)| over every case (tests/test_score_op_host.py asserts it): set by
# random-70x16257x128 with its host stand-in logits (|lse| ~ 15, where an fp32 ulp is 9.5e-7); twice that is a tenth of LSE_BAR
MEASURED_F32_LSE, MEASURED_F32_LSE_CASE = 8.5e-7, "random-70x16257x128"

MUTATIONS = ("last_valid_column_dropped", "pad_columns_counted", "halves_overlap_by_one", "upper_half_dropped", "merge_without_rescale",
             "tie_highest_index", "target_of_next_row", "target_init_zero", "tiles_beyond_64_dropped", "topk_from_best_tile_only",
             "topk_tie_order_by_descending_id", "topk_returns_pad_column", "far_tile_gives_nan")


# ---------------------------------------------------------------------------------------------------- mirrored routing and maps
def kcode(tile, wt=0):
    """csrc/kernels.h: GEMM_KCODE family 7"""
    return 7 | tile << 4 | wt << 13


def route(M, N, K, wt, cus=CUS):
    """launch_gemm_logsoftmax's record: the weight shape alone picks the family, M the orientation of k_gemm_g3"""
    nt = (N + 127) // 128
    if K >= 128 and nt >= 128:
        blocks = lambda bm, bn: ((M + bm - 1) // bm) * ((N + bn - 1) // bn)
        tall, wide = blocks(256, 128), blocks(128, 256)
        rt, rw = (tall + cus - 1) // cus, (wide + cus - 1) // cus
        use_wide = rw < rt or (rw == rt and wide < tall and M < 256)
        return kcode(7 if use_wide else 6, 1 if wt else 0)
    return kcode(3)


def family(code):
    return {3: "mfma", 6: "tall", 7: "wide"}[(code >> 4) & 15]


BLOCK = {"mfma": (64, 128), "tall": (256, 128), "wide": (128, 256)}         # rows x columns of a block tile


def mfma_col(wc, j, lane):
    return wc * 64 + j * 16 + (lane & 15)


def mfma_row(wr, i, lane, r):
    return wr * 32 + i * 16 + (lane >> 4) * 4 + r


def g3_col(wc, j, lane, r):
    return wc * 64 + j * 16 + (lane >> 4) * 4 + r


def g3_row(wr, i, lane):
    return wr * 64 + i * 16 + (lane & 15)


def tile_positions(fam):
    """(columns, rows) of a block tile as the epilogue's lanes hold them"""
    if fam == "mfma":
        cols = {mfma_col(wc, j, l) for wc in range(2) for j in range(4) for l in range(64)}
        rows = {mfma_row(wr, i, l, r) for wr in range(2) for i in range(2) for l in range(64) for r in range(4)}
    else:
        nwc = 2 if fam == "tall" else 4
        cols = {g3_col(wc, j, l, r) for wc in range(nwc) for j in range(4) for l in range(64) for r in range(4)}
        rows = {g3_row(wr, i, l) for wr in range(8 // nwc) for i in range(4) for l in range(64)}
    return cols, rows


# ---------------------------------------------------------------------------------------------------- fp32 orders of the chain
def _tree(x):
    """a butterfly over the last axis (a power of two): neighbours first"""
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _seq(x):
    """one accumulator from zero over the last axis, in order"""
    acc = np.zeros(x.shape[:-1], dtype=x.dtype)
    for i in range(x.shape[-1]):
        acc = acc + x[..., i]
    return acc


def _take_max(m, ix, om, oi, highest=False):
    take = (om > m) | ((om == m) & ((oi > ix) if highest else (oi < ix)))
    return np.where(take, om, m), np.where(take, oi, ix)


def ordered_top(z, ids, k, descending_id=False):
    """the k first of every row in the order (z descending, id ascending); z holds bf16 numbers or -inf, ids are < 2^31"""
    u = np.ascontiguousarray(z, dtype=np.float32).view(np.uint32)
    key = np.where(u >> 31 == 0, u ^ np.uint32(0x80000000), ~u) >> 16                     # monotone in z
    low = ids.astype(np.int64) if descending_id else INT_MAX - ids.astype(np.int64)
    comb = (key.astype(np.int64) << 32) | low
    part = -np.sort(np.partition(-comb, k - 1, axis=1)[:, :k], axis=1)
    low = part & 0xFFFFFFFF
    top = (low if descending_id else INT_MAX - low).astype(np.int64)
    return top


# ---------------------------------------------------------------------------------------------------- patterns
def lit_pattern(N, start, step=SPACING):
    p = np.zeros(N, dtype=np.float32)
    p[start % N::step] = LIT
    return p


def set_pattern(N, cols):
    p = np.zeros(N, dtype=np.float32)
    p[list(cols)] = LIT
    return p


def spread_pattern(N, T, anchor):
    """tile T holds the maximum; anchor = a lit column (the lit columns are those = anchor mod 67)"""
    nt = (N + 127) // 128
    g = -(-124 // max(1, nt - 1))
    t = np.arange(N) // 128
    d = np.minimum(np.abs(t - T) * g, 124)
    lit = (np.arange(N) % SPACING) == (anchor % SPACING)
    return (np.where(lit, LIT, 0.0) - 8.0 * d).astype(np.float32)


def tie_sets(N):
    nt = (N + 127) // 128
    last0 = (nt - 1) * 128
    sets = [[5, 6], [9, 13], [2, 18], [70, 86], [10, 74], [63, 64], [127, 128], [20, 20 + 128 * 3], [7, 64 * 128 + 7], [3 * 128 + 7, 67 * 128 + 7],
            [5 * 128 + 90, 70 * 128 + 1], [3 + 13 * i for i in range(9)], [200 + 131 * i for i in range(9)], [40 + SPACING * i for i in range(6)],
            [0, N - 1], [last0, N - 1], [last0 - 1, last0], [N - 2, N - 1]]
    out = []
    for s in sets:
        s = sorted({c for c in s if 0 <= c < N})
        if len(s) >= 2 and s not in out:
            out.append(s)
    return out


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)))


_Z_LAST = (None, None)      # the logits of the case used last (40 MB at the largest shape: one is kept)


class ScoreCase:
    def __init__(self, cls, M, N, K, patterns=(), toff=0, tag=""):
        self.cls, self.M, self.N, self.K, self.tag, self.toff = cls, M, N, K, tag, toff
        self.NT = (N + 127) // 128
        self._z = None
        lit_cols = None
        if cls in ("lit", "flat", "spread", "ties"):
            assert len(patterns) <= K - 2, (cls, M, N, K, len(patterns))
            W = torch.zeros(N, K)
            W[:, 0], W[:, 1] = LO
            for c, p in enumerate(patterns):
                W[:, 2 + c] = torch.from_numpy(p)
            self.base = np.array([1 if m % 5 == 3 else 0 for m in range(M)])
            self.pat = np.array([m % len(patterns) if len(patterns) else -1 for m in range(M)])
            A = torch.zeros(M, K)
            A[torch.arange(M), torch.from_numpy(self.base)] = 1.0
            if len(patterns):
                A[torch.arange(M), torch.from_numpy(2 + self.pat)] = 1.0
            self.A, self.W = A, W
            best = [np.nonzero(p == p.max())[0] for p in patterns]
            lit_cols = (lambda m: best[self.pat[m]]) if len(patterns) else None
        elif cls == "grid":
            g = _gen(M, N, K, 1)
            self.A = torch.randint(-4, 5, (M, K), generator=g).float()
            self.W = torch.randint(-4, 5, (N, K), generator=g).float() / 64
        else:
            g = _gen(M, N, K, 2)
            self.A = r64(torch.randn(M, K, generator=g)).float()
            self.W = r64(torch.randn(N, K, generator=g) * 0.3).float()
        self.targets = self._targets(lit_cols)
        self.ks = tuple(k for k in KS if k <= N)

    def _targets(self, lit_cols):
        """argmax / column 0 / column N - 1 / a lit column of an upper half / a sweep over the column positions (lit or not), by row"""
        M, N = self.M, self.N
        t = np.zeros(M, dtype=np.int32)
        f = 0
        for m in range(M):
            mc = lit_cols(m) if lit_cols else None
            kind = m % 8
            if kind == 0 and mc is not None:
                t[m] = mc[0]
            elif kind == 1:
                t[m] = 0 if (m // 8) % 2 == 0 else N - 1
            elif kind == 2 and mc is not None:
                up = mc[(mc % 128) >= 64]
                t[m] = up[(m // 8) % len(up)] if len(up) else mc[-1]
            else:
                n = (self.toff + f) % 256 + 256 * ((f * 3) % max(1, N // 256))
                t[m] = n % N
                f += 1
        return t

    @property
    def name(self):
        return f"{self.cls}-{self.M}x{self.N}x{self.K}" + (f"-{self.tag}" if self.tag else "")

    @property
    def exact(self):
        return self.cls != "random"

    def code(self, wt):
        return route(self.M, self.N, self.K, wt)

    @property
    def wts(self):
        """the g3 cases run with DTK_GEMM_WT off and on"""
        return (0, 1) if family(self.code(0)) != "mfma" else (0,)

    # ------------------------------------------------------------------------------------------ logits and the float64 reference
    def set_logits(self, z):
        """random class only: the device's own dtk_op_gemm logits (fp32 tensor of bf16 numbers) replace the host stand-in"""
        assert self.cls == "random"
        self._z = z.double()
        self.__dict__.pop("_ref", None)

    def dot64(self):
        return self.A.double() @ self.W.double().t()

    def z64(self):
        global _Z_LAST
        if self._z is not None:
            return self._z
        if _Z_LAST[0] is not self:
            _Z_LAST = (self, r64(self.dot64()))
        return _Z_LAST[1]

    def ref(self):
        """float64 of the operands: lse [M] float64; argmax, zmax, zt = z[target], top_ids / top_z [M][min(8, N)] as the device types"""
        if "_ref" not in self.__dict__:
            z = self.z64()
            zn = z.float().numpy()
            kk = min(8, self.N)
            top = ordered_top(zn, np.broadcast_to(np.arange(self.N), zn.shape), kk)
            rows = np.arange(self.M)
            self._ref = dict(lse=torch.logsumexp(z, dim=-1).numpy(), argmax=top[:, 0].astype(np.int32), zmax=zn[rows, top[:, 0]],
                             zt=zn[rows, self.targets], top_ids=top.astype(np.int32), top_z=zn[rows[:, None], top])
        return self._ref

    # ------------------------------------------------------------------------------------------ the chain, with or without a fault
    def chain(self, k=0, wt=0, dtype=np.float32, mutate=None, fam=None):
        assert mutate is None or mutate in MUTATIONS
        fam = fam or family(self.code(wt))
        M, N, NT = self.M, self.N, self.NT
        Np = NT * 128
        z = self.z64().numpy().astype(dtype)
        ninf = dtype(-np.inf)
        zp = np.full((M, Np), ninf, dtype=dtype)
        zp[:, :N] = z
        if mutate == "last_valid_column_dropped":
            zp[:, N - 1] = ninf
        if mutate == "pad_columns_counted":
            zp[:, N:] = z[:, N - 1:N]
        tg = self.targets.astype(np.int64)
        if mutate == "target_of_next_row":
            tg = tg[np.minimum(np.arange(M) + 1, M - 1)]
        highest = mutate == "tie_highest_index"
        ids = np.arange(Np, dtype=np.int64)
        T3 = zp.reshape(M, NT, 128)
        H = np.stack([T3[:, :, :64], T3[:, :, 63:127] if mutate == "halves_overlap_by_one" else T3[:, :, 64:]], axis=2)      # [M][NT][2][64]
        i3 = ids.reshape(NT, 128)
        idsH = np.stack([i3[:, :64], i3[:, 63:127] if mutate == "halves_overlap_by_one" else i3[:, 64:]], axis=1)[None]
        if mutate == "upper_half_dropped":
            H[:, :, 1, :] = ninf
        # ---- a wave's 64 columns of a row
        hm = H.max(-1)
        at = H == hm[..., None]
        hix = np.where(at, idsH, -1).max(-1) if highest else np.where(at, idsH, INT_MAX).min(-1)
        hix = np.where(hm == ninf, INT_MAX, hix)
        with np.errstate(invalid="ignore", over="ignore"):
            e = np.where(H == ninf, dtype(0), np.exp(H - np.where(hm == ninf, dtype(0), hm)[..., None])).astype(dtype)
        if fam == "mfma":           # a lane: columns j * 16 + c in j order; then the 16 lanes' butterfly
            hl = _tree(_seq(np.moveaxis(e.reshape(M, NT, 2, 4, 16), 3, -1)))
        else:                       # a lane: columns j * 16 + g * 4 + r in (j, r) order; then the four lanes g
            hl = _tree(_seq(np.moveaxis(e.reshape(M, NT, 2, 4, 4, 4), 4, 3).reshape(M, NT, 2, 4, 16)))
        hzt = np.where(idsH == tg[:, None, None, None], H, ninf).max(-1)
        del e, at
        # ---- ls_merge(lower half, upper half): a record
        rm, rix = _take_max(hm[:, :, 0], hix[:, :, 0], hm[:, :, 1], hix[:, :, 1], highest)
        with np.errstate(invalid="ignore"):
            part = [np.where(hm[:, :, h] == ninf, dtype(0), hl[:, :, h] * np.exp(hm[:, :, h] - rm)).astype(dtype) for h in (0, 1)]
        rl = part[0] + part[1]
        rzt = np.maximum(hzt[:, :, 0], hzt[:, :, 1])
        # ---- k_score_merge
        if mutate == "tiles_beyond_64_dropped":
            rm, rix, rl, rzt = rm[:, :64], rix[:, :64], rl[:, :64], rzt[:, :64]
        mx = rm.max(1)
        at = rm == mx[:, None]
        ix = np.where(at, rix, -1).max(1) if highest else np.where(at, rix, INT_MAX).min(1)
        zt = rzt.max(1)
        if mutate == "target_init_zero":
            zt = np.maximum(zt, dtype(0))
        with np.errstate(invalid="ignore"):
            w = np.exp(rm - mx[:, None]).astype(dtype)
            c = np.where(rm == ninf, dtype(0), rl if mutate == "merge_without_rescale" else rl * w).astype(dtype)
        if mutate == "far_tile_gives_nan":
            c = np.where((w == 0) & (rm != ninf), dtype(np.nan), c)
        trips = (c.shape[1] + 63) // 64
        cp = np.zeros((M, trips * 64), dtype=dtype)
        cp[:, :c.shape[1]] = c
        l = _tree(_seq(np.moveaxis(cp.reshape(M, trips, 64), 1, -1)))
        with np.errstate(invalid="ignore", divide="ignore"):
            lse = (mx + np.log(l)).astype(dtype)
        lse32 = lse.astype(np.float32)
        out = dict(lse=lse32, logprob=zt.astype(np.float32) - lse32, argmax=ix.astype(np.int32), zmax=mx.astype(np.float32))
        if k:
            # ---- k_score_top: the candidates are the valid columns (a padded lane reads lm_head's row N - 1 again: its z is NOT a candidate)
            zc = np.full((M, Np), -np.inf, dtype=np.float32)
            zc[:, :N] = z
            if mutate == "topk_returns_pad_column":
                zc[:, N:] = z[:, N - 1:N]
            if mutate == "topk_from_best_tile_only":
                keep = (ids[None, :] >> 7) == (ix[:, None] >> 7)
                zc = np.where(keep, zc, np.float32(-np.inf))
            top = ordered_top(zc, np.broadcast_to(ids, zc.shape), k, descending_id=mutate == "topk_tie_order_by_descending_id")
            tz = zc[np.arange(M)[:, None], top]
            out.update(top_ids=top.astype(np.int32), top_z=tz, top_logprob=tz - lse32[:, None])
        return out

    # ------------------------------------------------------------------------------------------ judging
    def judge(self, out, k=0):
        """out = the arrays of one call on all rows (lse, logprob, argmax, zmax, and top_ids, top_z, top_logprob [M][k] with k > 0).
        Returns (ok, figures)."""
        r = self.ref()
        lse = np.asarray(out["lse"], dtype=np.float32)
        fig = {"finite": bool(np.isfinite(lse).all() and np.isfinite(out["logprob"]).all() and np.isfinite(out["zmax"]).all())}
        fig["argmax"] = bool(np.array_equal(out["argmax"], r["argmax"]))
        fig["zmax"] = out["zmax"].tobytes() == r["zmax"].tobytes()
        with np.errstate(invalid="ignore"):
            d = np.abs(lse.astype(np.float64) - r["lse"])
            fig["d_lse"] = float(d.max()) if np.isfinite(d).all() else float("inf")
            fig["logprob"] = np.asarray(out["logprob"], dtype=np.float32).tobytes() == (r["zt"] - lse).tobytes()      # ONE fp32 subtraction
        ok = fig["finite"] and fig["argmax"] and fig["zmax"] and fig["logprob"] and fig["d_lse"] <= LSE_BAR
        if k:
            fig["top_ids"] = bool(np.array_equal(out["top_ids"], r["top_ids"][:, :k]))
            fig["top_z"] = out["top_z"].tobytes() == np.ascontiguousarray(r["top_z"][:, :k]).tobytes()
            with np.errstate(invalid="ignore"):
                fig["top_logprob"] = out["top_logprob"].tobytes() == (r["top_z"][:, :k] - lse[:, None]).tobytes()
            fig["top_finite"] = bool(np.isfinite(out["top_z"]).all() and np.isfinite(out["top_logprob"]).all())
            fig["top0"] = bool(np.array_equal(out["top_ids"][:, 0], out["argmax"]) and out["top_z"][:, 0].tobytes() == out["zmax"].tobytes())
            ok = ok and fig["top_ids"] and fig["top_z"] and fig["top_logprob"] and fig["top_finite"] and fig["top0"]
        return bool(ok), fig


# ---------------------------------------------------------------------------------------------------- the case list
MFMA_SHAPES = ((1, 8, 8), (65, 129, 8), (37, 257, 72), (64, 128, 64), (130, 8200, 64))
G3_SHAPES = ((70, 16257, 128), (257, 16257, 136), (300, 16384, 128), (129, 16512, 200))
PAIR = ((70, 16257, 128), (257, 16257, 128))          # wide against tall on the same lm_head: the first 70 rows are the same rows
FLAT_N = (129, 130, 255, 257, 1000)
_CACHE = {}


def _pair_starts():
    return [(254 + c) % 256 + 256 * ((c * 5) % 63) for c in range(69)] + [16256]      # + the ragged tile's only column


def _spread(M, N, K, toff):
    nt = (N + 127) // 128
    pats = []
    for i in range(min(K - 2, 12)):
        T = (0, nt // 2, nt - 1)[i % 3]
        lo, hi = T * 128, min(T * 128 + 128, N)
        pats.append(spread_pattern(N, T, lo + (i * 29) % (hi - lo)))
    return ScoreCase("spread", M, N, K, pats, toff)


def _ties(M, N, K, toff):
    return ScoreCase("ties", M, N, K, [set_pattern(N, s) for s in tie_sets(N)[:K - 2]], toff)


def all_cases():
    if "all" in _CACHE:
        return _CACHE["all"]
    lit = lambda M, N, K, starts, toff=0, tag="": ScoreCase("lit", M, N, K, [lit_pattern(N, s) for s in starts], toff, tag)
    cs = [
        # ---- k_gemm_mfma<64, 128, LS>
        lit(1, 8, 8, [3]),
        lit(65, 129, 8, [0, 63, 64, 127, 128, 5], 8),                                  # 128: the ragged tile's only column, argmax and target
        lit(37, 257, 72, [124 + c for c in range(36)] + [256], 40),
        lit(64, 128, 64, list(range(62)), 64),
        lit(130, 8200, 64, [62 + c + 128 * ((c * 11) % 64) for c in range(62)], 100),
        lit(5, 8192, 8, [8191, 100, 4100, 64, 8128, 127], 200),                        # NT = 64: the merge's one full trip
    ]
    cs += [ScoreCase("flat", M, N, K) for M, N, K in ((5, 129, 8), (3, 130, 8), (66, 255, 8), (2, 257, 16), (7, 1000, 8))]
    cs += [_spread(37, 257, 72, 3), _spread(130, 8200, 64, 77)]
    cs += [_ties(65, 129, 8, 17), _ties(64, 128, 64, 130), _ties(130, 8200, 64, 190)]
    cs += [ScoreCase("grid", M, N, K, toff=o) for (M, N, K), o in zip(MFMA_SHAPES, (0, 30, 90, 150, 210))]
    cs += [ScoreCase("random", 37, 1000, 64)]
    # ---- k_gemm_g3<LS>
    cs += [
        lit(70, 16257, 128, _pair_starts(), 0, "pair"),
        lit(257, 16257, 128, _pair_starts(), 0, "pair"),
        lit(257, 16257, 136, [c + 128 * ((c * 7) % 127) for c in range(134)], 20),
        lit(300, 16384, 128, [(c * 131 + 64) % 16384 for c in range(126)], 60),
        lit(129, 16512, 200, [(c * 257 + 100) % 16512 for c in range(129)], 90),
        lit(300, 16512, 256, [c + 256 * ((c * 7) % 64) for c in range(254)], 43, "wide"),      # 258 tall blocks need two rounds: the wide tile over three row blocks
    ]
    cs += [_spread(M, N, K, o) for (M, N, K), o in zip(G3_SHAPES, (86, 10, 50, 70))]
    cs += [_ties(M, N, K, o) for (M, N, K), o in zip(G3_SHAPES[:2] + G3_SHAPES[3:], (129, 30, 110))]
    cs += [ScoreCase("grid", M, N, K, toff=o) for (M, N, K), o in zip(G3_SHAPES, (172, 0, 64, 128))]
    cs += [ScoreCase("random", 70, 16257, 128, toff=215)]
    _CACHE["all"] = cs
    return cs


def cases_of(cls):
    return [c for c in all_cases() if c.cls == cls]


def pair_cases():
    a, b = [c for c in all_cases() if c.tag == "pair"]
    return a, b


CLASSES = ("lit", "flat", "spread", "ties", "grid", "random")
