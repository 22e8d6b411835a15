"""Oracle of classifier-free guidance (dtk_set_guidance), HF's UnbatchedClassifierFreeGuidanceLogitsProcessor:

    Lc = logsumexp(zc)   Lu = logsumexp(zu)   out[v] = g * ((zc[v] - Lc) - (zu[v] - Lu)) + (zu[v] - Lu)

`mix64` is the formula in float64.  `out32` is the device's float32 evaluation replayed on the host: given the DEVICE's (Lc, Lu) it
performs the same four operations per element in the same order, one IEEE rounding each (numpy float32 arithmetic never fuses a
multiply and an add), so it must reproduce the device's row bit for bit."""
from __future__ import annotations

from typing import Tuple

import numpy as np


def lse64(z) -> float:
    z = np.asarray(z, dtype=np.float64)
    m = float(z.max())
    return m + float(np.log(np.exp(z - m).sum()))


def mix64(zc, zu, g: float) -> Tuple[np.ndarray, float, float]:
    """(out, Lc, Lu) in float64"""
    zc, zu = np.asarray(zc, dtype=np.float64), np.asarray(zu, dtype=np.float64)
    Lc, Lu = lse64(zc), lse64(zu)
    lc, lu = zc - Lc, zu - Lu
    return float(g) * (lc - lu) + lu, Lc, Lu


def out32(zc, zu, g: float, Lc, Lu) -> np.ndarray:
    """float32, one rounding per operation: lc = zc - Lc; lu = zu - Lu; out = (g * (lc - lu)) + lu"""
    zc, zu = np.asarray(zc, dtype=np.float32), np.asarray(zu, dtype=np.float32)
    g, Lc, Lu = np.float32(g), np.float32(Lc), np.float32(Lu)
    lc = zc - Lc
    lu = zu - Lu
    d = lc - lu
    p = g * d
    out = p + lu
    assert out.dtype == np.float32
    return out


def logprob64(row, token: int) -> float:
    """float64 log-softmax of a (mixed) row at one token: what a guided step reports as its logprob"""
    return float(np.asarray(row, dtype=np.float64)[int(token)]) - lse64(row)
