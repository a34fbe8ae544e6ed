"""CPU: pins the float64 numpy references of tests/loss_np.py, which tests/test_gpu_losses.py holds the HIP kernels to.

focal_ref / orth_l1_ref against torch.autograd through oracle/model_torch.py (float64) on the small multi-level "layout" geometry:
the inputs are laid out in Keras order (B, N, C), the oracle's gradient is mapped back to the level-major rows with row_of().  Loss
and gradient agree to 1e-12 relative; for the gradient that is the strict measure of the GPU tests,
max |got - ref| / (|ref| + 1e-6 max |ref|) over EVERY element.  (A bare per-element ratio cannot hold 1e-12 in float64 on either
side: both form 1 - p by subtraction, which is good to 1.1e-16 absolute, i.e. 2e-11 relative at x = 12 and 4e-9 at x = 17.5;
measured here, the strict measure is below 4e-14.)
"""
import numpy as np
import pytest
import torch

from tests import loss_np as L

B, SHAPES = L.LAYOUT_B, L.LAYOUT_SHAPES
EPS, ONE_MINUS_EPS = 1e-7, 1 - 1e-7     # the oracle's constants (float64)
RTOL = 1e-12


def test_row_of_is_the_level_major_layout():
    """a permutation of the rows; level after level, image after image within a level, cells in order within an image"""
    rmap = L.row_of(B, SHAPES)
    cells = sum(h * w for h, w in SHAPES)
    assert rmap.shape == (B, cells) and sorted(rmap.reshape(-1).tolist()) == list(range(B * cells))
    assert rmap[0, 0] == 0 and rmap[1, 0] == 35 and rmap[2, 34] == 3 * 35 - 1      # level 0: 3 images of 35 cells
    assert rmap[0, 35] == 105 and rmap[1, 35] == 105 + 12 and rmap[2, 35 + 11] == 105 + 36 - 1   # level 1: 12 cells
    assert rmap[2, 35 + 12] == 141 + 2 * 4 and rmap[1, cells - 1] == 153 + 1 and rmap[2, cells - 1] == B * cells - 1
    k = np.arange(B * cells * 6, dtype=np.float64).reshape(B, cells * 2, 3)
    assert np.array_equal(L.to_keras(L.from_keras(k, B, SHAPES, 2, 3, 8, np.float64), B, SHAPES, 2, 3), k)


def oracle_focal(logits, y, A, C, alpha, gamma):
    from oracle import model_torch as MT
    x = torch.tensor(L.to_keras(logits, B, SHAPES, A, C).astype(np.float64), requires_grad=True)
    loss = MT.focal(torch.tensor(y.astype(np.float64)), torch.sigmoid(x), alpha, gamma)
    g, = torch.autograd.grad(loss, x)
    return float(loss.detach()), L.from_keras(g.numpy(), B, SHAPES, A, C, logits.shape[1], np.float64)


@pytest.mark.parametrize("saturate", [False, True], ids=["main", "clip-active"])
@pytest.mark.parametrize("alpha,gamma", [(0.25, 2.0), (0.4, 1.5), (0.25, 1.5), (0.4, 2.0)])
def test_focal_ref_matches_autograd_through_the_oracle(alpha, gamma, saturate):
    A, C, ld = 9, 13, 128
    logits, y = L.focal_inputs(np.random.default_rng(11), B, SHAPES, A, C, ld, saturate=saturate)
    count = int((y[:, :, C] == 1).sum())
    assert count > 0 and (y[:, :, C] == -1).any()
    want_loss, want = oracle_focal(logits, y, A, C, alpha, gamma)
    loss, d = L.focal_ref(logits, y, B, SHAPES, A, C, alpha, gamma, count, 1.0, EPS, ONE_MINUS_EPS)
    assert np.isfinite(d).all() and (d[:, A * C:] == 0).all()
    assert abs(loss - want_loss) <= RTOL * abs(want_loss)
    assert L.strict_measure(d, want) <= RTOL
    # the gradient carries loss_weight, the loss does not
    loss_h, d_h = L.focal_ref(logits, y, B, SHAPES, A, C, alpha, gamma, count, 0.5, EPS, ONE_MINUS_EPS)
    assert loss_h == loss and np.array_equal(d_h, 0.5 * d)
    if saturate:
        # where the clip is active the BCE does not move: what is left of the gradient is d(focal weight) * bce * p (1 - p)
        x = L.to_keras(logits, B, SHAPES, A, C).astype(np.float64)
        big = (np.abs(x) >= 17.5) & (y[:, :, C:] != -1)
        assert big.sum() > 100
        p = 1 / (1 + np.exp(-x))
        assert ((p[big] < EPS) | (p[big] > ONE_MINUS_EPS)).all()
        z = y[:, :, :C].astype(np.float64)
        q = np.where(z == 1, 1 - p, p)
        a_t = np.where(z == 1, alpha, 1 - alpha)
        pc = np.clip(p, EPS, ONE_MINUS_EPS)
        bce = -(z * np.log(pc) + (1 - z) * np.log(1 - pc))
        only_dfw = np.where(z == 1, -1.0, 1.0) * a_t * gamma * q ** (gamma - 1) * bce * p * (1 - p) / count
        got = L.to_keras(d, B, SHAPES, A, C)
        assert np.allclose(got[big], only_dfw[big], rtol=1e-12, atol=0)


@pytest.mark.parametrize("weight,sigma", [(0.125, 3.0), (0.3, 2.0), (0.125, 2.0)])
def test_orth_l1_ref_matches_autograd_through_the_oracle(weight, sigma):
    from oracle import model_torch as MT
    A, ld = 9, 160
    pred, y = L.orth_inputs(np.random.default_rng(12), B, SHAPES, A, ld)
    count = int((y[:, :, 16] == 1).sum())
    assert count > 0
    x = torch.tensor(L.to_keras(pred, B, SHAPES, A, 16).astype(np.float64), requires_grad=True)
    want_loss = MT.orthogonal_l1(torch.tensor(y.astype(np.float64)), x, weight, sigma)
    g, = torch.autograd.grad(want_loss, x)
    want_loss, want = float(want_loss.detach()), L.from_keras(g.numpy(), B, SHAPES, A, 16, ld, np.float64)
    loss, d = L.orth_l1_ref(pred, y, B, SHAPES, A, weight, sigma, count, 1.0)
    assert np.isfinite(d).all() and (d[:, A * 16:] == 0).all()
    assert abs(loss - want_loss) <= RTOL * abs(want_loss)
    assert L.strict_measure(d, want) <= RTOL
    loss_h, d_h = L.orth_l1_ref(pred, y, B, SHAPES, A, weight, sigma, count, 0.5)
    assert loss_h == loss and np.array_equal(d_h, 0.5 * d)
    # count 0: the normaliser is 1
    loss_1, d_1 = L.orth_l1_ref(pred, y, B, SHAPES, A, weight, sigma, 0, 1.0)
    assert abs(loss_1 - count * loss) <= RTOL * abs(loss_1) and L.strict_measure(d_1, count * d) <= RTOL


def test_orth_quadruples_are_the_twelve_edge_pairs():
    """each of the 8 corners (even index = its x) appears in 6 quadruples; each feature is a difference of two edge vectors, so it
    is blind to a translation of the box"""
    assert L.ORTH_QUADS.shape == (12, 4) and len({tuple(q) for q in L.ORTH_QUADS.tolist()}) == 12
    assert np.array_equal(np.bincount(L.ORTH_QUADS.reshape(-1), minlength=16), [6, 0] * 8)
    v = np.random.default_rng(0).standard_normal((5, 16))
    assert np.abs(L.orth_edges(v + 3.25) - L.orth_edges(v)).max() < 1e-12


def test_p16_stats_ref_on_hand_written_halves():
    h = np.zeros((40, 16), np.uint16)
    h[0, :6] = [0x0000, 0x8000, 0x3C00, 0xBC00, 0x0001, 0x83FF]    # +0, -0, 1, -1, smallest subnormal, largest subnormal (negative)
    h[1, :6] = [0x0400, 0x76FF, 0x7700, 0xF700, 0x7BFF, 0x7C00]    # smallest normal, just under the clamp, at it (+/-), 65504, inf
    h[1, 8:10] = [0x0200, 0x7A00]                                  # columns >= 8: a subnormal and a clamped one
    h[35, 0] = 0x7E00                                              # second 32-row block: a NaN pattern
    h[39, 15] = 0x03FF
    assert L.p16_stats_ref(h, 16) == (640, 14, 6, 4, 0x7E00)
    assert L.p16_stats_ref(h, 8) == (320, 11, 5, 2, 0x7E00)
    assert L.p16_stats_ref(h, 16, np.array([1, 0], np.uint8)) == (512, 12, 5, 3, 0x7C00)
    assert L.p16_stats_ref(h, 16, np.array([0, 1], np.uint8)) == (128, 2, 1, 1, 0x7E00)
    assert L.p16_stats_ref(h, 16, np.array([0, 0], np.uint8)) == (0, 0, 0, 0, 0)


def test_count_and_export_refs():
    rng = np.random.default_rng(5)
    y = np.zeros((2, 7, 4), np.float32)
    y[:, :, 3] = [[1, 0, -1, 1, 0, 0, 1], [0, 0, 0, -1, -1, 1, 0]]
    y[0, 1, 0] = 1.0                                               # a label in a background row is not a positive
    assert L.count_ref(y, None, np.zeros((1, 3, 2), np.float32), [5, 6, 7]).tolist() == [9, 6, 7]
    A, V, ld = 2, 3, 8
    src = rng.standard_normal((L.n_rows(B, SHAPES), ld)).astype(np.float32)
    src[:, A * V:] = np.nan
    out = L.export_ref(src, B, SHAPES, A, V, False)
    assert out.dtype == np.float32 and out.shape == (B, 52 * A, V)
    rmap = L.row_of(B, SHAPES)
    for b, cell, a, v in [(0, 0, 0, 0), (1, 34, 1, 2), (2, 35, 0, 1), (1, 50, 1, 0), (2, 51, 1, 2)]:
        assert out[b, cell * A + a, v] == src[rmap[b, cell], a * V + v]
    sig = L.export_ref(src, B, SHAPES, A, V, True)
    assert sig.dtype == np.float64 and np.allclose(sig, 1 / (1 + np.exp(-out.astype(np.float64))), rtol=1e-15)
