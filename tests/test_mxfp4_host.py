"""
MXFP4 on the CPU: the reference quantiser (tests/mxfp4_ref.py) on crafted blocks — the E2M1 ties, the block-scale rule at and just
above a mantissa of 1.5, an all-zero block, a ragged 16-element trailing block, the derived error bound — and the loader's refusal of
weight_format="mxfp4" with batch slots, which needs no GPU (it is raised before a context exists).
"""
import numpy as np
import pytest

from tests import mxfp4_ref as ref


def _row(vals, K=32):
    w = np.zeros((1, K))
    w[0, :len(vals)] = vals
    return w


def test_ties_round_to_the_even_code():
    # a block whose amax is 6 takes e = 0, so the values are the scaled values themselves
    vals = [6.0, 2.5, 3.5, 5.0, 0.25, 0.75, 1.25, 1.75, -2.5, -3.5, -5.0, -0.25, -0.75]
    want = [6.0, 2.0, 4.0, 4.0, 0.0, 1.0, 1.0, 2.0, -2.0, -4.0, -4.0, -0.0, -1.0]
    codes, scales, eff = ref.quantise(_row(vals))
    assert scales[0, 0] == 127
    assert np.array_equal(eff[0, :len(vals)], np.array(want))
    assert np.all(eff[0, len(vals):] == 0)
    for v, w in zip(vals, want):                       # the per-element statement of the rule agrees with the vectorised path
        assert ref.GRID[ref.e2m1_code(abs(v))] == abs(w)
    # nibble order: weight 2i in the low nibble of byte i, 2i + 1 in the high one; sign in bit 3
    assert codes[0, 0] == (7 | (4 << 4))               # 6.0 -> code 7, 2.5 -> 2.0 = code 4
    assert codes[0, 4] == ((4 | 8) | ((6 | 8) << 4))   # -2.5 -> -2 (code 4 + sign), -3.5 -> -4 (code 6 + sign)
    assert np.array_equal(ref.dequantise(codes, scales, 32), eff)
    # the same ties at another scale (e = -20 and e = +8): powers of two move nothing
    for e in (-20, 8):
        c2, s2, eff2 = ref.quantise(_row(vals) * 2.0 ** e)
        assert s2[0, 0] == 127 + e and np.array_equal(c2, codes) and np.array_equal(eff2, eff * 2.0 ** e)


def test_block_scale_at_and_above_mantissa_one_and_a_half():
    # amax = m * 2^E: e = E - 2, one more if m > 1.5 (6 = 1.5 * 2^2 is the largest E2M1 value)
    assert ref.block_exp(6.0) == 0 and ref.block_exp(1.5) == -2 and ref.block_exp(1.5 * 2.0 ** 10) == 8
    just_above = float(np.float32(1.5) + np.float32(2.0 ** -7))          # the next bf16 above 1.5
    assert ref.block_exp(just_above) == -1 and ref.block_exp(just_above * 4) == 1
    assert ref.block_exp(1.0) == -2 and ref.block_exp(1.9921875) == -1 and ref.block_exp(2.0) == -1 and ref.block_exp(4.0) == 0
    for amax in (1.5, just_above, 1.0, 0.0072021484375, 3.0, 448.0, 2.0 ** -100):
        e = ref.block_exp(amax)
        assert amax * 2.0 ** -e <= 6.0 < amax * 2.0 ** -(e - 1)           # the smallest such e
    # at m == 1.5 the largest weight is kept exactly (scaled to 6); just above it is scaled to 3.0x and rounds to 3
    _, s, eff = ref.quantise(_row([1.5, 0.1]))
    assert s[0, 0] == 125 and eff[0, 0] == 1.5
    _, s, eff = ref.quantise(_row([just_above, 0.1]))
    assert s[0, 0] == 126 and eff[0, 0] == 1.5                            # 3.015625 -> 3 at e = -1


def test_all_zero_block_and_ragged_trailing_block():
    codes, scales, eff = ref.quantise(np.zeros((2, 64)))
    assert np.all(scales == 127) and np.all(codes == 0) and np.all(eff == 0)
    # K = 48: the second block has 16 real weights; its amax is theirs alone and its padding is zero codes
    rng = np.random.default_rng(0)
    W = rng.standard_normal((3, 48)) * 0.05
    W[:, :32] *= 64.0                                                     # a large first block must not leak into the second one's scale
    codes, scales, eff = ref.quantise(W)
    assert codes.shape == (3, 32) and scales.shape == (3, 2) and eff.shape == (3, 48)
    assert np.all(codes[:, 24:] == 0)
    for n in range(3):
        assert scales[n, 1] == 127 + ref.block_exp(float(np.abs(W[n, 32:]).max()))
        assert scales[n, 0] > scales[n, 1]
    alone = ref.quantise(W[:, 32:])
    assert np.array_equal(alone[2], eff[:, 32:]) and np.array_equal(alone[0][:, :8], codes[:, 16:24])
    assert np.array_equal(ref.dequantise(codes, scales, 48), eff)


@pytest.mark.parametrize("K", [32, 48, 688, 2080])
def test_error_bound_is_a_quarter_of_the_block_amax(K):
    """The scaled amax lies in (3, 6].  Above 4 the widest gap of the grid (4 .. 6) applies: error <= 1 scaled = amax / 4 at most
    (amax > 4); below, the widest gap is 1 (2 .. 3, 3 .. 4): error <= 0.5 <= amax / 6.  So |W_eff - W| <= 0.25 * amax of the block."""
    rng = np.random.default_rng(K)
    W = rng.standard_normal((16, K)) * np.exp2(rng.integers(-12, 6, size=(16, 1)).astype(np.float64))
    W[3] = 0.0
    W[5, ::7] = 0.0
    _, scales, eff = ref.quantise(W)
    for c in range((K + 31) // 32):
        blk, q = W[:, c * 32:(c + 1) * 32], eff[:, c * 32:(c + 1) * 32]
        amax = np.abs(blk).max(axis=1, keepdims=True)
        assert np.all(np.abs(q - blk) <= 0.25 * amax)
        assert np.all(np.abs(q).max(axis=1, keepdims=True) <= 6.0 * np.exp2(scales[:, c:c + 1].astype(np.float64) - 127))   # never saturates
        assert np.all(np.sign(q) * np.sign(blk) >= 0)
    # values on the grid times the block's power of two are kept exactly (element 0 of every block is 6 * 2^e: that pins its scale)
    KC = (K + 31) // 32
    e_blk = rng.integers(-20, 9, size=(8, KC))
    Wg = rng.choice(np.concatenate([ref.GRID, -ref.GRID]), size=(8, KC * 32)) * np.repeat(np.exp2(e_blk.astype(np.float64)), 32, axis=1)
    Wg[:, ::32] = 6.0 * np.exp2(e_blk.astype(np.float64))
    Wg = Wg[:, :K]
    _, scales, eff = ref.quantise(Wg)
    assert np.array_equal(scales, (e_blk + 127).astype(np.uint8)) and np.array_equal(eff, Wg)


def test_load_refuses_mxfp4_with_batch_slots():
    """MXFP4 weights stream in single-sequence decode only: load() says so before it creates a context (no GPU needed)"""
    from detikzify_amd.model import load
    with pytest.raises(NotImplementedError, match="batched-slot or multi-vector"):
        load("detikzify-tiny", synthetic=1, weight_format="mxfp4", batch_slots=2)
