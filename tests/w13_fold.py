"""What tests/test_w13_fold_host.py and tests/test_gpu_w13_shapes.py share: the RMSNorm prologue's fold of k_gemv mirrored in float32
numpy, the 13-bit shapes of kernels_decode.hip's launch_gemv_w13_variant with their bf16 twins, and the K = 4096 / 4104 cases with the
seeds at which the fold of 4 waves and the fold of a block's own 8 or 16 waves give another `inv`."""
from __future__ import annotations

import numpy as np

from tests import gemv_cases as gc

# 13-bit shape -> (R, U, waves, blocks per CU of the persistent grid | 0, waves that fold the norm)
_PAIRED13 = {0: (1, 4, 4, 0, 4), 1: (2, 4, 4, 0, 4), 2: (1, 4, 8, 0, 8), 3: (1, 4, 8, 2, 8), 4: (1, 8, 4, 0, 4), 5: (1, 4, 4, 4, 4),
             6: (1, 4, 8, 2, 4), 7: (1, 4, 16, 1, 4)}
TABLE13 = {
    (gc.RMSNORM, gc.QKV): _PAIRED13,
    (gc.RMSNORM, gc.SWIGLU): _PAIRED13,
    (gc.COPY, gc.RESID): {0: (1, 8, 8, 0, 0), 1: (1, 4, 8, 0, 0), 2: (2, 4, 4, 0, 0), 3: (1, 4, 8, 0, 0), 4: (2, 4, 8, 0, 0), 5: (1, 4, 4, 0, 0), 6: (1, 4, 16, 0, 0)},
    (gc.RMSNORM, gc.LOGITS): {0: (1, 4, 4, 0, 4), 1: (2, 4, 4, 0, 4), 2: (1, 4, 8, 2, 8), 3: (2, 4, 8, 2, 8), 4: (2, 4, 8, 0, 8),
                              5: (2, 4, 8, 2, 4), 6: (1, 4, 8, 2, 4), 7: (2, 4, 16, 1, 4)},
    (gc.RMSNORM, gc.STORE): {0: (2, 4, 4, 0, 4), 1: (2, 4, 8, 2, 4)},
}
# the shapes whose fold is not their block's: shape -> the bf16 variant with that fold (4 waves)
NEW = {
    (gc.RMSNORM, gc.QKV): {6: 0, 7: 0},
    (gc.RMSNORM, gc.SWIGLU): {6: 0, 7: 0},
    (gc.RMSNORM, gc.LOGITS): {5: 3, 6: 3, 7: 3},
    (gc.RMSNORM, gc.STORE): {1: -1},
}
# every 13-bit shape of the four roles of the zero-code cases -> a bf16 variant of equal fold (K <= 2048: every wave count folds alike)
TWIN = {
    (gc.RMSNORM, gc.SWIGLU): {**{v: 0 for v in range(8)}, 2: 10, 3: 10},
    (gc.COPY, gc.RESID): {0: -1, 1: -1, 2: -1, 3: 13, 4: 14, 5: -1, 6: -1},
    (gc.RMSNORM, gc.LOGITS): {0: 3, 1: 3, 2: 1, 3: 1, 4: 1, 5: 3, 6: 3, 7: 3},
    (gc.RMSNORM, gc.QKV): {**{v: 0 for v in range(8)}, 2: 10, 3: 10},
}

# (role, keyword arguments of gemv_cases.Case, seed): found by tests/test_w13_fold_host.py's search (python -m tests.w13_fold)
NORM_CASES = [
    ((gc.RMSNORM, gc.SWIGLU), dict(K=4096, ff=24), 4),
    ((gc.RMSNORM, gc.SWIGLU), dict(K=4104, ff=24), 47),
    ((gc.RMSNORM, gc.LOGITS), dict(K=4096, N=37), 169),
    ((gc.RMSNORM, gc.LOGITS), dict(K=4104, N=37), 364),
    ((gc.RMSNORM, gc.STORE), dict(K=4096, N=37), 342),
    ((gc.RMSNORM, gc.STORE), dict(K=4104, N=37), 64),
    ((gc.RMSNORM, gc.QKV), dict(K=4096, H=32, KVH=1, hd=128), 44),
    ((gc.RMSNORM, gc.QKV), dict(K=4096, H=64, KVH=1, hd=64), 6),
]


def case_x(role, kw, seed):
    """the x of gemv_cases.Case(role, "bf16", **kw, seed=seed) without its weights (Case draws x first from its generator)"""
    import torch
    from oracle.ops import rb
    pro, epi = role
    K, hd = kw["K"], kw.get("hd", 128)
    N = kw.get("N", 0) if epi in (gc.STORE, gc.RESID, gc.LOGITS) else ((kw["H"] + 2 * kw["KVH"]) * hd if epi == gc.QKV else 2 * kw["ff"])
    g = torch.Generator().manual_seed(100003 * pro + 1009 * epi + 7 * K + 31 * N + 13 * kw.get("S", 0) + hd + seed)
    return rb(torch.randn(K, generator=g)).numpy().astype(np.float32)


def fold_tot(x, fw, one_pass=None):
    """k_gemv's PRO_RMSNORM sum of squares when fw waves fold: thread t of fw * 64 adds the squares of chunks t, t + fw * 64, ... (8
    values each, in order, 16 per step of the one-pass form), wave_sum's xor butterfly 32, 16, .., 1, then the waves in order.  one_pass:
    True / False forces the form (the one-pass form holds chunks t and t + fw * 64 only), None takes the kernel's choice."""
    x = np.asarray(x, dtype=np.float32)
    K8, FT = x.size // 8, fw * 64
    if one_pass is None:
        one_pass = K8 <= 2 * FT
    assert not one_pass or K8 <= 2 * FT
    rounds = 2 if one_pass else -(-K8 // FT)
    ch = np.zeros((rounds * FT, 8), np.float32)          # chunks behind the end: zeros, whose squares change no sum
    ch[:K8] = x.reshape(K8, 8)
    ss = np.zeros(FT, np.float32)
    for r in range(rounds):
        for e in range(8):
            v = ch[r * FT:(r + 1) * FT, e]
            ss = (ss + v * v).astype(np.float32)         # (v * v is exact: bf16 values)
    lanes = ss.reshape(fw, 64)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[:, np.arange(64) ^ off]).astype(np.float32)
    tot = np.float32(0.0)
    for w in range(fw):
        tot = np.float32(tot + lanes[w, 0])
    return tot


def inv_of(tot, K, eps=gc.EPS):
    """rsqrtf(tot / K + eps): the argument in float32 as the kernel forms it, its inverse root rounded once"""
    var = np.float32(np.float32(tot / np.float32(K)) + np.float32(eps))
    return np.float32(1.0 / np.sqrt(np.float64(var)))


def inv_bits(x, fw, one_pass=None):
    return int(inv_of(fold_tot(x, fw, one_pass), np.asarray(x).size).view(np.uint32))


def packable(role, kw, seed):
    """every row of the case's matrix packs (no weight more than 30 binades below its row's largest): the op would stream bf16 rows otherwise"""
    import ctypes as C
    from detikzify_amd import _lib
    from oracle.ops import f32_to_bits
    lib = _lib.load_library()
    W = np.ascontiguousarray(f32_to_bits(gc.Case(role[0], role[1], "bf16", seed=seed, **kw).W))
    N, K = W.shape
    planes, hb, bad = np.zeros((N, lib.dtk_w13_row_bytes(K)), np.uint8), np.zeros(N, np.uint8), np.zeros(N, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.dtk_w13_pack_host(p(W), N, K, p(planes), p(hb), p(bad)) == 0
    return not bad.any()


def search(role, kw, seeds=range(400)):
    """the seed at which the 4-wave fold is furthest (in ulps of the sum) from both the 8- and the 16-wave fold, `inv` differing from
    both, among the seeds whose matrix packs"""
    found = []
    for seed in seeds:
        x = case_x(role, kw, seed)
        t = [fold_tot(x, fw).view(np.uint32).astype(np.int64) for fw in (4, 8, 16)]
        i = [inv_bits(x, fw) for fw in (4, 8, 16)]
        if i[0] != i[1] and i[0] != i[2]:
            found.append((int(min(abs(t[0] - t[1]), abs(t[0] - t[2]))), seed))
    for d, seed in sorted(found, key=lambda f: (-f[0], f[1])):
        if packable(role, kw, seed):
            return d, seed
    return None


if __name__ == "__main__":
    for role, kw, _ in NORM_CASES:
        print(gc.PRO_NAME[role[0]], gc.EPI_NAME[role[1]], kw, search(role, kw))
