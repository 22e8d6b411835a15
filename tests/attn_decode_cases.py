"""Inputs and the float64 reference of the decode-attention op tests (tests/test_attn_decode_host.py checks them on the CPU,
tests/test_gpu_attn_decode.py feeds the same objects to dtk_op_attn_decode / dtk_op_attn_decode_b).

Random keys give a near-uniform softmax: one key dropped or counted twice out of n moves a head output by ~1 / n, below any bar.  A
SPOTLIGHT input makes one key of a query head hold >= 0.99 of the float64 probability mass: K[kvh, j*] = rb(alpha * q[h]), so the
head output is V[kvh, j*] (every V row is distinct: randn + 0.01 * j) unless the kernel scores exactly the keys of the reference.
Several positions run against one cache, so a head's spotlight keys form a LADDER: key i of the sorted ladder scores S0 + i * DELTA,
each one outweighs everything below it, and at position p the spotlit key is the largest ladder key <= p.  A ladder key just above
the position is a trap: a kernel that lets one row past the context in lands on a key that outweighs the whole context.
Rows the kernel must not read at all hold POISON: finite, +-3e4."""
from __future__ import annotations

import math

import torch

from oracle.ops import rb

POSITIONS = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 598, 599]
SPLITS = [1, 2, 3, 4, 16]
H = 8
T_MAX = 600
# the position lists of one call: rows above a call's largest position are poison, so the list is cut where that still leaves rows
POSITION_GROUPS = [[p for p in POSITIONS if p <= 257], [511, 512, 513, 598], [599]]
# (threads, mode) pairs the context's options allow: contiguous splits (threads 0) have no head_dim-64 kernel
CONFIGS_128 = [(0, 0), (0, 1), (0, 2), (0, 3), (256, 0), (256, 2), (512, 0), (512, 2), (1024, 0), (1024, 2)]
CONFIGS_64 = [(256, 0), (256, 2), (512, 0), (512, 2), (1024, 0), (1024, 2)]
S0, DELTA = 16.0, 7.0          # score of a ladder's first key, and the step to the next: exp(-7) of the mass leaks one step down
MASS = 0.99
POISON = 3e4

B_T_MAX = 320
B_POSITIONS = [0, 15, 16, 1, 17, 63, 64, 65, 127, 255, 128, 129, 256, 257, 319, 300]     # slots 3 and 9 are the inactive ones
B_SHARE_LENS = [3, 4, 63, 64, 65, 153, 256]


def tile_rows(threads, hd):
    """keys per tile of the single-sequence kernels: k_attn_decode_t deals tiles of 16 (hd 128) / 32 (hd 64) rows per wave; the
    contiguous-split kernel (threads 0) walks its range 64 rows at a time"""
    return 64 if threads == 0 else (threads // 4 if hd == 128 else threads // 2)


def second_split_first_key(threads, hd, S, pos):
    """first key of split 1, or None when the position leaves it empty"""
    if S < 2:
        return None
    if threads:
        k = tile_rows(threads, hd)
    else:
        k = (((pos + 1 + S - 1) // S) + 15) & ~15
    return k if k <= pos else None


def ortho_q(Hq, KVH, hd, g):
    """bf16-rounded randn query heads; the heads that share a K/V head are made orthogonal first (Gram-Schmidt, norms kept), so that a
    spotlight key of one head scores ~0 for the others of its group"""
    q = torch.randn(Hq, hd, generator=g, dtype=torch.float64)
    G = Hq // KVH
    for k in range(KVH):
        for a in range(G):
            h = k * G + a
            n = q[h].norm()
            for b in range(a):
                o = q[k * G + b]
                q[h] -= (q[h] @ o) / (o @ o) * o
            q[h] *= n / q[h].norm()
    return rb(q.float())


def attn_ref(q, K, V, pos):
    """float64 softmax attention of one query token: q [H][hd], K / V [KVH][T][hd], keys 0..pos of kv head h // G.  Returns
    (out [H][hd], probs [H][pos + 1])"""
    Hq, hd = q.shape
    G = Hq // K.shape[0]
    k = K[:, :pos + 1].double().repeat_interleave(G, dim=0)
    v = V[:, :pos + 1].double().repeat_interleave(G, dim=0)
    s = torch.einsum("hd,hjd->hj", q.double(), k) * hd ** -0.5
    p = torch.softmax(s, dim=-1)
    return torch.einsum("hj,hjd->hd", p, v), p


def random_cache(KVH, T, hd, g):
    K = rb(torch.randn(KVH, T, hd, generator=g))
    V = rb(torch.randn(KVH, T, hd, generator=g) + 0.01 * torch.arange(T, dtype=torch.float32)[None, :, None])
    return K, V


def set_ladders(K, q, ladders, rows):
    """adds the ladders {head: keys} to K [KVH][T][hd].  rows {(kvh, key): float64 row} collects what the spotlight rows hold: a key
    that several heads of one K/V head spotlight is the SUM of their alpha * q[h] — the heads are orthogonal (ortho_q), so each sees its
    own term.  Returns {head: sorted keys}."""
    Hq, hd = q.shape
    G = Hq // K.shape[0]
    done = {}
    for h, keys in ladders.items():
        kvh = h // G
        mine = sorted(k for k in set(keys) if 0 <= k < K.shape[1])
        unit = float(q[h].double() @ q[h].double()) * hd ** -0.5        # score of the key q[h] itself
        for i, k in enumerate(mine):
            rows[(kvh, k)] = rows.get((kvh, k), 0) + q[h].double() * ((S0 + i * DELTA) / unit)
            K[kvh, k] = rb(rows[(kvh, k)].float())
        done[h] = mine
    return done


def poison(K, V, rows, flavour):
    """rows: boolean [T] (or index) of rows the kernel must not read; two flavours that differ in every element"""
    a = POISON if flavour == 0 else -0.75 * POISON
    n = K.shape[-1]
    pat = torch.where(torch.arange(n) % 2 == 0, torch.tensor(a), torch.tensor(-a))
    K[:, rows] = rb(pat)
    V[:, rows] = rb(-pat)


def assert_spots(probs_of, spots):
    """spots {(…, head): key}; probs_of(...) -> float64 probabilities [H][n].  A miss is a bug of the test input."""
    for key, j in spots.items():
        p = probs_of(*key[:-1])[key[-1]]
        assert j < p.numel() and float(p[j]) >= MASS, f"spotlight {key} -> key {j}: mass {float(p[j]) if j < p.numel() else None}"


# ------------------------------------------------------------------------------------------ single sequence
class SingleCase:
    """one call of dtk_op_attn_decode: q, K, V (and K2 / V2: the same with other poison above the last position), the positions, the
    float64 reference per position and the spotlit key of every (position index, head) that has one"""

    def __init__(self, hd, KVH, positions, threads, S, seed, spotlight=True):
        g = torch.Generator().manual_seed(seed)
        self.hd, self.KVH, self.positions = hd, KVH, list(positions)
        self.q = ortho_q(H, KVH, hd, g)
        self.K, self.V = random_cache(KVH, T_MAX, hd, g)
        ladders = {}
        if spotlight:
            R, P = tile_rows(threads, hd), self.positions
            ladders[1] = [0]                                                        # key 0
            ladders[0] = [k for p in P for k in (p - 1, p, p + 1)]                  # key pos (and the trap at pos + 1)
            ladders[2] = [(p // R) * R for p in P]                                  # first key of the last tile
            ladders[3] = [k for k in (second_split_first_key(threads, hd, S, p) for p in P) if k is not None]
            order = sorted(POSITIONS)
            ladders[4] = [p - 1 for p in P if order.index(p) % 2 == 0]              # key pos - 1, for every other position:
            ladders[5] = [p - 1 for p in P if order.index(p) % 2 == 1]              # neighbouring positions would outweigh each other
        self.ladders = set_ladders(self.K, self.q, ladders, {})
        above = torch.arange(T_MAX) > max(self.positions)
        self.K2, self.V2 = self.K.clone(), self.V.clone()
        poison(self.K, self.V, above, 0)
        poison(self.K2, self.V2, above, 1)
        ref = [attn_ref(self.q, self.K, self.V, p) for p in self.positions]
        self.ref = torch.stack([r[0] for r in ref])                                  # [npos][H][hd]
        self.probs = [r[1] for r in ref]
        self.spots = {}
        for i, p in enumerate(self.positions):
            for h, keys in self.ladders.items():
                vis = [k for k in keys if k <= p]
                if vis:
                    self.spots[(i, h)] = max(vis)
        assert_spots(lambda i: self.probs[i], self.spots)

    def wants(self):
        """which of the issue's spotlight kinds this case holds, as {kind: count} (the host test checks none is empty overall)"""
        out = {"pos": 0, "pos-1": 0, "key0": 0, "tile": 0, "split2": 0}
        for (i, h), k in self.spots.items():
            p = self.positions[i]
            out["pos"] += h == 0 and k == p
            out["pos-1"] += h in (4, 5) and k == p - 1
            out["key0"] += h == 1 and k == 0
            out["tile"] += h == 2
            out["split2"] += h == 3
        return out


def single_cases(hd, KVH, threads, S):
    return [SingleCase(hd, KVH, P, threads, S, seed=1000 * hd + 10 * KVH + i) for i, P in enumerate(POSITION_GROUPS)]


def single_random_case(hd, KVH):
    return SingleCase(hd, KVH, POSITIONS, 0, 1, seed=7 * hd + KVH, spotlight=False)


def combine_partials(pm, pl, po):
    """float64 flash-decode reduction of [H][S] / [H][S] / [H][S][hd] partials"""
    pm, pl, po = pm.double(), pl.double(), po.double()
    w = torch.exp(pm - pm.max(dim=1, keepdim=True).values)
    return (w[..., None] * po).sum(1) / (w * pl).sum(1)[:, None]


# ------------------------------------------------------------------------------------------ batched
class BatchCase:
    """one call of dtk_op_attn_decode_b.  slots: list of dicts {pos, active, src (-1), L (0)}; heads 0..3 of every slot share one q so
    that a spotlight key in a source's cache works for all of its forks.  spot(s) -> {head: key} declares a slot's spotlights in its
    EFFECTIVE cache (rows < L of the source, the rest its own); keys of heads 0 and 1 below L go to the source's cache as ladders."""

    def __init__(self, KVH, slots, seed, rows=64, spotlight=True):
        g = torch.Generator().manual_seed(seed)
        n = len(slots)
        self.KVH, self.slots, self.n = KVH, slots, n
        T, hd = B_T_MAX, 128
        qs = ortho_q(H, KVH, hd, g)
        self.q = torch.stack([ortho_q(H, KVH, hd, g) for _ in range(n)])
        self.q[:, :4] = qs[:4]
        # heads 0..3 are shared, 4..7 per slot: re-orthogonalising is not needed across kv groups, only inside one; with G = 4 the
        # groups are {0..3} (all shared) and {4..7} (all per slot), with G = 2 likewise pairs; G = 1 has nothing to keep apart
        self.K = torch.empty(n, KVH, T, hd)
        self.V = torch.empty(n, KVH, T, hd)
        for s in range(n):
            self.K[s], self.V[s] = random_cache(KVH, T, hd, g)
        self.pos = [sl["pos"] for sl in slots]
        self.active = [int(sl.get("active", 1)) for sl in slots]
        self.src = [sl.get("src", -1) for sl in slots]
        self.L = [sl.get("L", 0) if sl.get("src", -1) >= 0 else 0 for sl in slots]
        self.spots = {}
        if spotlight:
            taken = [{} for _ in range(n)]
            src_ladders = {}                                   # source slot -> {head: keys}
            for s, sl in enumerate(slots):
                if self.src[s] >= 0:
                    lad = src_ladders.setdefault(self.src[s], {1: [0], 0: []})
                    lad[0] += [self.L[s] - 1, self.L[s]]       # key L - 1, and the trap at L: the source's row L is not the fork's
            for s0, lad in src_ladders.items():
                set_ladders(self.K[s0], self.q[s0], lad, taken[s0])
            for s, sl in enumerate(slots):
                if not self.active[s]:
                    continue
                p, L = self.pos[s], self.L[s]
                own = {}
                if self.src[s] >= 0:
                    own = {2: [L], 3: [p]}                     # first private key, last key
                elif s not in src_ladders:
                    own = {0: [p], 1: [rows] if rows <= p else [], 2: [2 * rows] if 2 * rows <= p else []}
                else:
                    own = {3: [p]}
                set_ladders(self.K[s], self.q[s], own, taken[s])
        # poison: a fork's own rows below L, every slot's rows above what it or its forks may read
        top = list(self.pos)
        for s in range(n):
            if not self.active[s]:
                top[s] = -1
        for s in range(n):
            if self.src[s] >= 0 and self.active[s]:
                top[self.src[s]] = max(top[self.src[s]], self.L[s] - 1)
        for s in range(n):
            r = torch.arange(T)
            bad = r > top[s]
            if self.src[s] >= 0:
                bad |= r < self.L[s]
            poison(self.K[s], self.V[s], bad, 0)
        self.ref = torch.zeros(n, H, hd, dtype=torch.float64)
        self.probs = {}
        for s in range(n):
            if not self.active[s]:
                continue
            Ke, Ve = self.effective(s)
            self.ref[s], self.probs[s] = attn_ref(self.q[s], Ke, Ve, self.pos[s])
        if spotlight:
            G = H // KVH
            for s in range(n):
                if not self.active[s]:
                    continue
                p, L = self.pos[s], self.L[s]
                if self.src[s] >= 0:
                    want = {0: L - 1, 1: 0, 2: L, 3: p}
                elif s in src_ladders:
                    want = {1: 0, 3: p}
                else:
                    want = {0: p, 1: rows, 2: 2 * rows}
                for h, k in want.items():
                    if 0 <= k <= p:
                        self.spots[(s, h)] = k
            assert_spots(lambda s: self.probs[s], self.spots)

    def effective(self, s):
        """the cache slot s attends over: rows < L from its source"""
        Ke, Ve = self.K[s], self.V[s]
        if self.src[s] >= 0 and self.L[s] > 0:
            Ke, Ve = Ke.clone(), Ve.clone()
            Ke[:, :self.L[s]] = self.K[self.src[s]][:, :self.L[s]]
            Ve[:, :self.L[s]] = self.V[self.src[s]][:, :self.L[s]]
        return Ke, Ve

    def own_rows_ref(self, s):
        """the deliberately WRONG reference of a fork: its own rows instead of the source's"""
        return attn_ref(self.q[s], self.K[s], self.V[s], self.pos[s])[0]


def private_lengths(rows):
    return [1, 2, rows - 1, rows, rows + 1, 2 * rows + 1, 3 * rows + 1]


def unshared_case(KVH, rows):
    slots = [{"pos": p, "active": int(i not in (3, 9))} for i, p in enumerate(B_POSITIONS)]
    return BatchCase(KVH, slots, seed=31 * KVH + rows, rows=rows)


def shared_cases(KVH, rows):
    """slot 0 = the source (it decodes too, at the last position); every (L, private length) that fits T_max as a fork, 15 per call"""
    forks = [(L, n) for L in B_SHARE_LENS for n in private_lengths(rows) if n >= 1 and L + n <= B_T_MAX]
    forks = list(dict.fromkeys(forks))
    cases = []
    for i in range(0, len(forks), 15):
        slots = [{"pos": B_T_MAX - 1}] + [{"pos": L + n - 1, "src": 0, "L": L} for L, n in forks[i:i + 15]]
        slots += [{"pos": 0, "active": 0}] * (16 - len(slots))
        cases.append(BatchCase(KVH, slots, seed=977 * KVH + rows + i, rows=rows))
    return cases


def grouping_case(KVH=4):
    """64 slots: source 0 (idle) with 17 forks (a group of 16 and a singleton), source 20 (idle) with 2 forks, source 24 that decodes
    itself with one fork, six slots that share nothing, the rest idle"""
    idle = {"pos": 0, "active": 0}
    slots = [dict(idle) for _ in range(64)]
    for s in range(1, 18):
        slots[s] = {"pos": 153 + s, "src": 0, "L": 153}
    slots[21] = {"pos": 70, "src": 20, "L": 64}
    slots[22] = {"pos": 200, "src": 20, "L": 64}
    slots[24] = {"pos": 250}
    slots[25] = {"pos": 65, "src": 24, "L": 65}
    for s, p in zip(range(40, 46), (0, 31, 32, 33, 64, 319)):
        slots[s] = {"pos": p}
    return BatchCase(KVH, slots, seed=4242, rows=32)


def sub_case(case, n, only):
    """the first n slots of a case with only slot `only` active: same arrays, so the slot's bits must not move"""
    return [case.pos[s] for s in range(n)], [int(s == only) for s in range(n)], case.src[:n], case.L[:n]
