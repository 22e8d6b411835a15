"""Inputs of the MXFP8 key/value op tests: the batched cases of tests/attn_decode_cases.py (imported, not edited) with a kv8_from
boundary per slot.  Rows [from, pos) of an active slot live in the shadow planes (oracle.llama.mx_quantise of the bf16 rows) and are
POISON in the bf16 cache handed to the kernel; row pos stays bf16 there and is NaN (0xFF, as a code and as a scale) in the shadow, like
every shadow row the kernel must not read: below from, above pos, idle slots, a fork's shared range.  The float64 reference attends over
the de-quantised rows [from, pos] — the row of the step itself included.

tests/test_kv8_host.py checks on the CPU that these inputs keep their teeth, tests/test_gpu_kv8_attn.py feeds them to
dtk_op_attn_decode_b8."""
from __future__ import annotations

import numpy as np
import torch

from oracle.llama import mx_fake_quant, mx_quantise
from oracle.ops import f32_to_bits
from tests import attn_decode_cases as ac

MODES = ("L", "mid", "tile-", "tile", "tile+", "pos")      # where kv8_from sits between the slot's share_len and its position
NAN8 = 0xFF


def boundaries(case, mode, rows):
    """kv8_from per slot.  lo = the slot's share_len, or for a source the largest share_len of its forks (they read its bf16 rows below
    that); "L" = lo, "pos" = only the new row, "mid" halfway, "tile" / "tile-" / "tile+" = the first tile edge above lo (tiles of
    `rows` keys counted from lo) and the rows beside it, clipped into [lo, pos]."""
    lo = list(case.L)
    for s in range(case.n):
        if case.src[s] >= 0 and case.active[s]:
            lo[case.src[s]] = max(lo[case.src[s]], case.L[s])
    out = []
    for s in range(case.n):
        p = case.pos[s]
        l = min(lo[s], p)
        f = {"L": l, "pos": p, "mid": (l + p) // 2, "tile-": l + rows - 1, "tile": l + rows, "tile+": l + rows + 1}[mode]
        out.append(max(l, min(p, f)))
    return out


class Kv8Case:
    """a BatchCase + boundaries: .Kin / .Vin (bf16 caches for the kernel, rows [from, pos) poisoned), .k8 / .k8s / .v8 / .v8s (shadow
    planes as uint8 arrays), .ref (float64, de-quantised rows), .probs, .want (codes and scales of row pos per active slot)"""

    def __init__(self, case, mode, rows):
        self.case, self.mode = case, mode
        n, KVH, T = case.n, case.KVH, ac.B_T_MAX
        self.frm = boundaries(case, mode, rows)
        self.Kin, self.Vin = case.K.clone(), case.V.clone()
        self.Kdq, self.Vdq = case.K.clone(), case.V.clone()          # what the reference sees of every slot's OWN rows
        self.k8 = np.full((n, KVH, T, 128), NAN8, dtype=np.uint8)
        self.v8 = np.full((n, KVH, T, 128), NAN8, dtype=np.uint8)
        self.k8s = np.full((n, KVH, T, 4), NAN8, dtype=np.uint8)
        self.v8s = np.full((n, KVH, T, 4), NAN8, dtype=np.uint8)
        self.want = {}
        for s in range(n):
            if not case.active[s]:
                continue
            f, p = self.frm[s], case.pos[s]
            for X, Xin, Xdq, c8, s8, tag in ((case.K, self.Kin, self.Kdq, self.k8, self.k8s, "k"), (case.V, self.Vin, self.Vdq, self.v8, self.v8s, "v")):
                own = X[s][:, f:p + 1]
                codes, scales = mx_quantise(own, 32)
                Xdq[s][:, f:p + 1] = mx_fake_quant(own, 32)
                c8[s][:, f:p] = codes[:, :p - f].numpy()
                s8[s][:, f:p] = scales[:, :p - f].numpy()
                self.want[(s, tag)] = (codes[:, p - f].numpy(), scales[:, p - f].numpy())
            if p > f:
                ac.poison(self.Kin[s], self.Vin[s], torch.arange(f, p), 1)
        self.ref = torch.zeros(n, ac.H, 128, dtype=torch.float64)
        self.probs = {}
        for s in range(n):
            if case.active[s]:
                Ke, Ve = self.effective(s)
                self.ref[s], self.probs[s] = ac.attn_ref(case.q[s], Ke, Ve, case.pos[s])

    def effective(self, s):
        """rows < L from the source's BF16 cache (shared rows are never MXFP8), the rest the slot's own, de-quantised from kv8_from on"""
        c = self.case
        Ke, Ve = self.Kdq[s], self.Vdq[s]
        if c.src[s] >= 0 and c.L[s] > 0:
            Ke, Ve = Ke.clone(), Ve.clone()
            Ke[:, :c.L[s]] = c.K[c.src[s]][:, :c.L[s]]
            Ve[:, :c.L[s]] = c.V[c.src[s]][:, :c.L[s]]
        return Ke, Ve

    def bits(self):
        if not hasattr(self, "_bits"):
            self._bits = tuple(f32_to_bits(x) for x in (self.case.q, self.Kin, self.Vin))
        return self._bits

    def distance(self):
        """rel-L2 between the reference on the de-quantised rows and the bf16 one, over the active slots"""
        a = torch.tensor([bool(x) for x in self.case.active])
        d = (self.ref[a] - self.case.ref[a]).norm() / self.case.ref[a].norm()
        return float(d)
