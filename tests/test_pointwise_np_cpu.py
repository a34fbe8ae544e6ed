"""CPU: the host restatements of tests/pointwise_np.py against closed forms (hand-computed tables, the oracle's upsample rule,
the transpose of the gather matrix, one Adam step by hand).  The GPU tests hold the kernels to these functions, so these
functions are held to something that is not a program of ours."""
import numpy as np
import torch

from tests import pointwise_np as PN


def test_maxpool_by_hand():
    # 3x3, all negative: 'same' pads one row / column BEFORE (total 2) -- windows rows {-1,0,1}, {1,2,3}; a zero pad would win
    x = -(np.arange(9, dtype=np.float32) + 1).reshape(1, 3, 3, 1)
    assert PN.tf_same(3) == (1, 1, 2)
    assert np.array_equal(PN.maxpool3x3s2(x)[0, :, :, 0], np.array([[-1, -2], [-4, -5]], np.float32))
    # 4x5: rows pad (0, 1) -> windows {0,1,2}, {2,3}; columns pad (1, 1) -> windows {0,1}, {1,2,3}, {3,4}
    img = np.array([[1, 9, 2, 8, 3], [7, 0, 6, 1, 5], [4, 4, 4, 4, 4], [-1, -2, -3, -4, 10]], np.float32)
    assert PN.tf_same(4) == (0, 1, 2) and PN.tf_same(5) == (1, 1, 3)
    assert np.array_equal(PN.maxpool3x3s2(img.reshape(1, 4, 5, 1))[0, :, :, 0], np.array([[9, 9, 8], [4, 4, 10]], np.float32))
    # channels and images are independent; -inf survives only where the whole window is -inf
    two = np.stack([img, -img], axis=-1)[None]
    got = PN.maxpool3x3s2(np.concatenate([two, two[:, ::-1]], axis=0))
    assert np.array_equal(got[0, :, :, 0], [[9, 9, 8], [4, 4, 10]]) and np.array_equal(got[0, :, :, 1], [[0, 0, -1], [2, 4, 4]])
    assert np.array_equal(got[1, :, :, 0], PN.maxpool3x3s2(img[::-1].reshape(1, 4, 5, 1).copy())[0, :, :, 0])
    inf = np.full((1, 3, 3, 1), -np.inf, np.float32)
    inf[0, 2, 2, 0] = 5
    assert np.array_equal(PN.maxpool3x3s2(inf)[0, :, :, 0], [[-np.inf, -np.inf], [-np.inf, 5]])


def test_upsample_index_tables_match_the_oracle():
    from oracle import model_torch as MT
    for n_in, n_out in ((17, 34), (23, 45)):
        idx = PN.nn_index(n_in, n_out)
        src = torch.arange(n_in, dtype=torch.float64).reshape(1, 1, n_in, 1)
        like = torch.zeros((1, 1, n_out, 1))
        assert np.array_equal(MT.upsample_like(src, like)[0, 0, :, 0].numpy(), idx.astype(np.float64))
    assert np.array_equal(PN.nn_index(17, 34), np.arange(34) // 2)  # integer factor: plain repetition
    # 23 -> 45: floor((d + 0.5) * 23 / 45) in integers (never within 1/90 of a whole number, so float32 cannot move it)
    assert np.array_equal(PN.nn_index(23, 45), [(2 * d + 1) * 23 // 90 for d in range(45)])
    assert PN.nn_index(23, 45)[-1] == 22 and PN.nn_index(2, 5).tolist() == [0, 0, 1, 1, 1] and PN.nn_index(6, 3).tolist() == [1, 3, 5]


def test_upsample_bwd_is_the_transpose_of_the_gather():
    rng = np.random.default_rng(0)
    for s in range(1, 13):
        for t in range(1, 25):
            G = PN.gather_matrix(s, t)  # [t, s]
            assert np.array_equal(G.sum(1), np.ones(t))
            # rows: (s -> t) with one column; columns: (s -> t) with one row; integers, so every sum is exact in float32
            g = rng.integers(-8, 9, size=(2, t, 1, 3)).astype(np.float32)
            want = np.einsum("ts,btxc->bsxc", G, g.astype(np.float64))
            assert np.array_equal(PN.upsample_add_bwd(g, s, 1), want.astype(np.float32))
            gT = np.ascontiguousarray(g.transpose(0, 2, 1, 3))
            assert np.array_equal(PN.upsample_add_bwd(gT, 1, s), want.transpose(0, 2, 1, 3).astype(np.float32))
            # forward = the gather itself
            src = rng.integers(-8, 9, size=(2, s, 1, 3)).astype(np.float32)
            assert np.array_equal(PN.upsample_add_fwd(src, t, 1), np.einsum("ts,bsxc->btxc", G, src).astype(np.float32))
    # both axes at once, with a base, in float64: <up(src), g> == <src, bwd(g)> and bwd(g, base) == base + bwd(g)
    src, g, base = rng.standard_normal((2, 5, 7, 4)), rng.standard_normal((2, 11, 16, 4)), rng.standard_normal((2, 5, 7, 4))
    adj = PN.upsample_add_bwd(g, 5, 7, dtype=np.float64)
    want = np.einsum("ty,ux,btuc->byxc", PN.gather_matrix(5, 11), PN.gather_matrix(7, 16), g)
    assert np.abs(adj - want).max() < 1e-13
    assert np.abs(PN.upsample_add_bwd(g, 5, 7, base=base, dtype=np.float64) - (base + want)).max() < 1e-13
    assert abs((PN.upsample_add_fwd(src, 11, 16) * g).sum() - (src * adj).sum()) < 1e-11
    other = rng.standard_normal((2, 11, 16, 4))
    assert np.array_equal(PN.upsample_add_fwd(src, 11, 16, other), PN.upsample_add_fwd(src, 11, 16) + other)


def test_upsample_bwd_float32_order():
    """the float32 form adds base, then the target pixels row-major: shown on values where the order changes the result"""
    big, one = np.float32(2 ** 24), np.float32(1)
    g = np.array([big, one, one, -big], np.float32).reshape(1, 2, 2, 1)  # 1x1 <- 2x2: ((big + 1) + 1) - big = 0 in float32
    assert PN.upsample_add_bwd(g, 1, 1)[0, 0, 0, 0] == 0.0
    assert PN.upsample_add_bwd(g, 1, 1, dtype=np.float64)[0, 0, 0, 0] == 2.0
    base = np.full((1, 1, 1, 1), -big, np.float32)
    g2 = np.array([big, one, one, one], np.float32).reshape(1, 2, 2, 1)  # (((-big + big) + 1) + 1) + 1 = 3: the base goes first
    assert PN.upsample_add_bwd(g2, 1, 1, base=base)[0, 0, 0, 0] == 3.0


def test_bwd_search_window_contains_the_preimage():
    """the backward kernels look for the target pixels of source pixel sy in int(sy * t/s) - 2 .. int((sy + 1) * t/s) + 2 (float32),
    clamped to the target: for every size pair the GPU tests use (s <= 47, t <= 96) that window holds the whole preimage, so the
    adjoint restated here and the kernels' search add the same pixels"""
    for s in range(1, 48):
        for t in range(1, 97):
            idx, sy = PN.nn_index(s, t), np.arange(s)
            inv = np.float32(t) / np.float32(s)
            lo = np.maximum((sy.astype(np.float32) * inv).astype(np.int64) - 2, 0)
            hi = np.minimum(((sy + 1).astype(np.float32) * inv).astype(np.int64) + 2, t - 1)
            first, last = np.searchsorted(idx, sy, side="left"), np.searchsorted(idx, sy, side="right") - 1
            some = first <= last
            assert np.all(first[some] >= lo[some]) and np.all(last[some] <= hi[some]), (s, t)


def test_packers_by_hand():
    x3 = np.arange(2 * 2 * 3 * 3, dtype=np.float32).reshape(2, 2, 3, 3) + 1
    out = PN.pack_rgb_padded(x3, 5, 6, 2)
    assert out.shape == (2, 5, 6, 4) and np.array_equal(out[:, 2:4, 2:5, :3], x3)
    assert out.sum() == x3.sum() and np.all(out[..., 3] == 0)
    u8 = np.full((2, 2, 3, 3), 200, np.uint8)
    u8[1, 0, 0] = (0, 128, 255)
    pre = PN.preprocess_caffe_u8_padded(u8, [(2, 3), (1, 1)], 4, 5, 1)
    want = np.float32(200) - np.array([103.939, 116.779, 123.68], np.float32)
    assert np.array_equal(pre[0, 1:3, 1:4, :3], np.broadcast_to(want, (2, 3, 3))) and np.all(pre[0, 0] == 0) and np.all(pre[..., 3] == 0)
    assert np.array_equal(pre[1, 1, 1, :3], np.array([0, 128, 255], np.float32) - np.array([103.939, 116.779, 123.68], np.float32))
    assert np.count_nonzero(pre[1]) == 3  # image 1 is 1 x 1: the rest of its frame stays 0.0, not -mean
    assert not PN.preprocess_caffe_u8_padded(u8, [(0, 0), (0, 0)], 4, 5, 1).any()


def test_adam_step_by_hand():
    P = PN.Param
    lr, b1, b2 = 1e-3, 0.9, 0.999
    # one scaled tensor, two columns: effective gradient g * scale = (0.6, -0.2); first Adam step moves every weight by lr * sign
    params = [P(0, 2, 2, 1, 0, 0.0)]
    w0, g, sc = np.array([1.0, -1.0]), np.array([0.3, -0.4]), np.array([2.0, 0.5])
    w, weff, m, v, norm = PN.adam_clipnorm_step(params, w0, np.zeros(2), np.zeros(2), g, sc, lr, b1, b2, 0.0, 0.0, 1)
    assert abs(norm - np.sqrt(0.4)) < 1e-15
    assert np.allclose(m, [0.06, -0.02], rtol=1e-14) and np.allclose(v, [3.6e-4, 4e-5], rtol=1e-14)
    assert np.allclose(w, [1.0 - lr, -1.0 + lr], rtol=1e-14) and np.allclose(weff, w * sc, rtol=1e-15)
    # second step from that state: lr_t = lr * sqrt(1 - b2^2) / (1 - b1^2)
    w2, _, m2, v2, _ = PN.adam_clipnorm_step(params, w, m, v, g, sc, lr, b1, b2, 1e-7, 0.0, 2)
    m_want, v_want = 0.9 * 0.06 + 0.1 * 0.6, 0.999 * 3.6e-4 + 0.001 * 0.36
    assert abs(m2[0] - m_want) < 1e-15 and abs(v2[0] - v_want) < 1e-17
    assert abs(w2[0] - (w[0] - lr * np.sqrt(1 - b2 ** 2) / (1 - b1 ** 2) * m_want / (np.sqrt(v_want) + 1e-7))) < 1e-15
    # the clip: norm >= clipnorm scales the gradient to norm clipnorm (keras: >=, so equality clips, by a factor 1); below, untouched
    _, _, mc, vc, nc = PN.adam_clipnorm_step(params, w0, np.zeros(2), np.zeros(2), g, sc, lr, b1, b2, 0.0, 0.1, 1)
    assert abs(nc - np.sqrt(0.4)) < 1e-15 and np.allclose(mc, np.array([0.06, -0.02]) * 0.1 / np.sqrt(0.4), rtol=1e-14)
    assert np.allclose(vc, np.array([3.6e-4, 4e-5]) * 0.01 / 0.4, rtol=1e-14)
    _, _, mn, _, _ = PN.adam_clipnorm_step(params, w0, np.zeros(2), np.zeros(2), g, sc, lr, b1, b2, 0.0, 10.0, 1)
    assert np.allclose(mn, [0.06, -0.02], rtol=1e-14)
    # L2: + 2 * l2 * w in the gradient and in the norm; the per-column scale index is e % ld on a 2 x 2 tensor; a frozen tensor
    # between them keeps w, m, v, adds nothing to the norm and still gets w_eff = w * scale; the gap (element 3) is left alone
    params = [P(0, 3, 3, 1, -1, 0.5), P(4, 2, 1, 0, 2, 0.25), P(6, 4, 2, 1, 0, 0.0)]
    w0 = np.array([1.0, 2.0, -1.0, 77.0, 3.0, 4.0, 1.0, 1.0, 1.0, 1.0])
    g = np.array([0.0, 1.0, 1.0, 55.0, 9.0, 9.0, 1.0, 1.0, 2.0, 2.0])
    sc = np.array([2.0, 0.5, 10.0])
    ge = PN.effective_grad(params, w0, g, sc)
    assert np.array_equal(ge, [1.0, 3.0, 0.0, 0.0, 0.0, 0.0, 2.0, 0.5, 4.0, 1.0])
    assert PN.l2_penalty(params, w0) == 0.5 * 6.0
    m0, v0 = np.full(10, 0.25), np.full(10, 0.5)
    w, weff, m, v, norm = PN.adam_clipnorm_step(params, w0, m0, v0, g, sc, lr, b1, b2, 1e-7, 0.0, 1)
    assert abs(norm - np.sqrt(1 + 9 + 4 + 0.25 + 16 + 1)) < 1e-14
    assert np.array_equal(w[3:6], w0[3:6]) and np.array_equal(m[3:6], m0[3:6]) and np.array_equal(v[3:6], v0[3:6])
    assert np.array_equal(weff[4:6], [30.0, 40.0]) and np.isnan(weff[3])
    assert np.allclose(m[6:], 0.9 * 0.25 + 0.1 * np.array([2.0, 0.5, 4.0, 1.0]), rtol=1e-15)
    assert np.allclose(weff[6:], w[6:] * np.array([2.0, 0.5, 2.0, 0.5]), rtol=1e-15) and np.array_equal(weff[:3], w[:3])
    assert m[2] == 0.9 * 0.25 and w[2] < w0[2]  # zero gradient: the moment decays and still moves the weight
