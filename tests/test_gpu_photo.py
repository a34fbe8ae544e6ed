"""GPU: the photometric augmentation kernels (pp_photo_augment_u8, pyrapose_amd/csrc/photo.hip) against their numpy restatement
(tests/photo_np.py).  The definitions are float32 + - * / in a stated order with host-built tables, compiled without
contraction: the device bytes must EQUAL the restatement's."""
import numpy as np
import pytest
import torch

from tests import photo_np as PN

pytestmark = pytest.mark.gpu

# (H, W): the two training shapes, an odd-sized image, and one smaller than a 64 x 16 tile plus its halo
SIZES = [(480, 640), (540, 720), (97, 131), (13, 21)]


@pytest.fixture(scope="module")
def ctx():
    from pyrapose_amd.runtime import default_context
    return default_context()


def _images(seed, B, H, W):
    """noise on top of smooth ramps: blurs, medians and the HSV branches all see both flat and busy neighbourhoods"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(xx * 255 // max(W - 1, 1)), (yy * 255 // max(H - 1, 1)), ((xx + yy) % 256)], axis=-1)
    img = np.empty((B, H, W, 3), np.uint8)
    for b in range(B):
        noise = rng.integers(-60, 61, size=(H, W, 3))
        img[b] = np.clip(np.roll(base, b, axis=-1) * (b % 3 != 2) + noise + 128 * (b % 3 == 2), 0, 255)
    img[:, : H // 4, : W // 4] = rng.integers(0, 256, size=(B, H // 4, W // 4, 3))  # a fully random corner
    return img


def single_ops():
    """18 ops, each alone (run as batches of 8 different programs)"""
    from pyrapose_amd.utils import photometric as PH
    rng = np.random.default_rng(77)
    m = PH.frequency_noise_mask(rng, -2.0, 12)
    return [
        PH.op_lut(PH.compose_luts(PH.lut_add([4, -9, 10]), PH.lut_gamma([0.8, 1.0, 1.2]))),
        PH.op_gray(0.2),
        PH.op_huesat(7, -12),
        PH.op_huesat(-11, 15),
        PH.op_blend(PH.lut_multiply([0.75, 1.25, 1.1]), PH.lut_linear_contrast(1.3), m),
        PH.op_blend(PH.lut_multiply(1.2), PH.lut_linear_contrast([0.7, 1.0, 1.3]), rng.uniform(size=(32, 5)).astype(np.float32)),
        PH.op_conv(PH.gaussian_taps(0.7)),
        PH.op_conv(PH.gaussian_taps(1.9)),
        PH.op_conv(PH.average_taps(3)),
        PH.op_conv(PH.average_taps(6)),
        PH.op_conv(PH.motion_taps(7, 31.0, 0.6)),
        PH.op_median(3),
        PH.op_median(5),
        PH.op_median(7),
        PH.op_bilateral(*PH.bilateral_tables(3, 25.0, 80.0)),
        PH.op_bilateral(*PH.bilateral_tables(7, 120.0, 15.0)),
        PH.op_bilateral(*PH.bilateral_tables(5, 10.0, 250.0)),
        PH.op_conv(np.array([[1.0]], np.float32)),
    ]


def run(ctx, img, chains, fuse=True):
    from pyrapose_amd import ops
    from pyrapose_amd.utils import photometric as PH
    progs = PH.compile_chain(chains, fuse=fuse)
    got = ops.photo_augment_u8(ctx, torch.from_numpy(img).cuda(), progs)
    torch.cuda.synchronize()
    return got.cpu().numpy(), progs


def assert_same(got, want, what):
    if not np.array_equal(got, want):
        diff = got.astype(int) - want.astype(int)
        bad = np.argwhere(diff != 0)
        raise AssertionError("%s: %d of %d bytes differ (max |d| %d), first at %s: got %d want %d" % (
            what, len(bad), diff.size, np.abs(diff).max(), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize("hw", SIZES)
def test_each_op_alone_is_byte_identical(ctx, hw):
    H, W = hw
    all_ops = single_ops()
    for lo in range(0, len(all_ops), 8):
        ops8 = all_ops[lo:lo + 8]
        img = _images(lo, len(ops8), H, W)
        got, _ = run(ctx, img, [[op] for op in ops8])
        for b, op in enumerate(ops8):
            assert_same(got[b], PN.apply_op(img[b], op), "%dx%d op %d (%s)" % (H, W, lo + b, op["kind"]))


@pytest.mark.parametrize("hw", SIZES)
def test_each_op_alone_batch_of_one(ctx, hw):
    H, W = hw
    all_ops = single_ops()
    for i in (2, 4, 10, 13, 15):
        img = _images(100 + i, 1, H, W)
        got, _ = run(ctx, img, [[all_ops[i]]])
        assert_same(got[0], PN.apply_op(img[0], all_ops[i]), "%dx%d B=1 op %d" % (H, W, i))


@pytest.mark.parametrize("hw", SIZES)
def test_sampled_chains_are_byte_identical(ctx, hw):
    from pyrapose_amd.utils import photometric as PH
    H, W = hw
    rng = np.random.default_rng(H * 1000 + W)
    for B in (8, 1):
        chains = [PH.sample_chain(rng) for _ in range(B)]
        img = _images(B, B, H, W)
        got, progs = run(ctx, img, chains)
        for b in range(B):
            assert_same(got[b], PN.apply_chain(img[b], progs.chains[b]), "%dx%d B=%d image %d %s" % (
                H, W, B, b, [op["kind"] for op in progs.chains[b]]))


def test_long_and_empty_programs(ctx):
    """stage slots and ping-pong: three neighbourhood ops in a row, a run of per-pixel ops longer than one launch carries, an
    empty program (a copy), unfused adjacent LUTs -- all in one batch"""
    from pyrapose_amd.utils import photometric as PH
    s = single_ops()
    chains = [
        [s[13], s[7], s[16]],
        [s[1], s[2], s[1], s[3], s[4], s[1], s[0], s[2], s[5]],
        [],
        [s[0], s[0], s[0]],
        [s[11], s[1], s[2], s[0], s[4], s[3], s[10], s[0]],
        [s[14]],
    ]
    for H, W in ((97, 131), (64, 128), (480, 640)):
        img = _images(9, len(chains), H, W)
        for fuse in (True, False):
            got, progs = run(ctx, img, chains, fuse=fuse)
            for b in range(len(chains)):
                assert_same(got[b], PN.apply_chain(img[b], chains[b]), "%dx%d fuse=%s image %d" % (H, W, fuse, b))
        assert np.array_equal(got[2], img[2])


def test_batch_larger_than_one_launch_carries(ctx):
    """more than 32 images go through in two launches per stage slot (the stage records travel as kernel arguments)"""
    s = single_ops()
    for B in (33, 64):
        chains = [[s[(3 * b) % len(s)], s[(b + 1) % 6]] if b % 5 else [] for b in range(B)]
        chains[B - 1] = [s[13], s[4], s[16]]
        img = _images(B, B, 24, 40)
        got, _ = run(ctx, img, chains, fuse=False)
        for b in range(B):
            assert_same(got[b], PN.apply_chain(img[b], chains[b]), "B=%d image %d" % (B, b))
    from pyrapose_amd import ops
    from pyrapose_amd.utils import photometric as PH
    with pytest.raises(ValueError):
        ops.photo_augment_u8(ctx, torch.zeros((65, 8, 8, 3), dtype=torch.uint8, device="cuda"), PH.compile_chain([[]] * 65))


def test_images_of_a_batch_are_independent_and_runs_repeat(ctx):
    from pyrapose_amd.utils import photometric as PH
    H, W = 97, 131
    rng = np.random.default_rng(31)
    chains = [PH.sample_chain(rng) for _ in range(8)]
    img = _images(4, 8, H, W)
    got, _ = run(ctx, img, chains)
    again, _ = run(ctx, img, chains)
    assert np.array_equal(got, again)
    for b in range(8):
        alone, _ = run(ctx, img[b:b + 1], [chains[b]])
        assert np.array_equal(alone[0], got[b]), b
    H, W = 480, 640
    img = _images(5, 8, H, W)
    got, _ = run(ctx, img, chains)
    again, _ = run(ctx, img, chains)
    assert np.array_equal(got, again)
    alone, _ = run(ctx, img[5:6], [chains[5]])
    assert np.array_equal(alone[0], got[5])


def test_malformed_programs_raise_before_any_launch(ctx):
    from pyrapose_amd import ops
    from pyrapose_amd.utils import photometric as PH
    img = torch.from_numpy(_images(0, 1, 32, 48)).cuda()
    out = torch.full_like(img, 7)
    good = PH.compile_chain([[PH.op_conv(PH.average_taps(3)), PH.op_lut(PH.lut_add(3))]])

    def broken(**fields):
        p = PH.compile_chain([[PH.op_conv(PH.average_taps(3)), PH.op_lut(PH.lut_add(3))]])
        for k, (i, v) in fields.items():
            p.ops[k][i] = v
        return p
    for p in (broken(k=(0, 4)), broken(k=(0, 9)), broken(kind=(1, 42)), broken(kind=(1, 0)), broken(off0=(1, good.pool.size)),
              broken(off0=(0, good.pool.size - 8)), broken(off0=(1, -4)), broken(off0=(1, 2)), broken(kind=(0, 6), k=(0, 1))):
        with pytest.raises(ValueError):
            ops.photo_augment_u8(ctx, img, p, out=out)
    with pytest.raises(ValueError):  # a channel count other than 3
        ops.photo_augment_u8(ctx, torch.zeros((1, 32, 48, 4), dtype=torch.uint8, device="cuda"), good)
    with pytest.raises(ValueError):  # one program per image
        ops.photo_augment_u8(ctx, torch.zeros((2, 32, 48, 3), dtype=torch.uint8, device="cuda"), good)
    torch.cuda.synchronize()
    assert bool((out == 7).all())  # nothing was launched
    ops.photo_augment_u8(ctx, img, good, out=out)
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy()[0], PN.apply_chain(img.cpu().numpy()[0], good.chains[0]), "good program")


def test_engine_step_with_photometric_programs(ctx):
    """train_step_from_annotations(photometric=P, transforms=T) takes the step of the same feed given the host-restated
    augmented images with transforms=T; photometric=None is the step as it was.  Bounds: those of
    test_gpu_api.test_train_step_from_annotations_equals_the_numpy_feed for one step reached through two feeds (the loss
    sums are float32 atomics: two runs of the SAME step differ by up to ~1.3e-6 relative)."""
    import bench
    from pyrapose_amd import arch, ops
    from pyrapose_amd.engine import Engine
    from pyrapose_amd.utils import photometric as PH
    from tests.test_gpu_image import random_transform
    B, H, W, C = 2, 96, 128, 5
    rng = np.random.default_rng(5)
    _, images, anns = bench.synth_batch(B, H, W, C, seed=3, side=(20, 50))
    u8 = _images(3, B, H, W)
    Wt = arch.init_weights(C, seed=4)
    mats = [random_transform(rng, H, W) for _ in range(B)]
    s = single_ops()
    progs = PH.compile_chain([[s[7], s[2], s[0], s[4]], [s[15], s[1], s[0]]])

    def step(img, photometric, look_ahead=False):
        eng = Engine(ctx, C, B, H, W, weights=Wt, train=True)
        t = torch.from_numpy(img).cuda()
        nb = dict(images_u8=t, transforms=mats, photometric=photometric) if look_ahead else None
        eng.train_step_from_annotations(t, anns, transforms=mats, photometric=photometric, next_batch=nb)
        torch.cuda.synchronize()
        first = (eng.losses(), eng.params.w_master.clone())
        if look_ahead:  # the second step consumes the prefetched (augmented, warped) prefix
            eng.train_step_from_annotations(t, anns, transforms=mats, photometric=photometric)
            torch.cuda.synchronize()
            first = (eng.losses(), eng.params.w_master.clone())
        eng.close()
        return first

    def same(a, b):
        for k in a[0]:
            assert abs(a[0][k] - b[0][k]) <= 4e-6 * max(abs(b[0][k]), 1e-6), (k, a[0][k], b[0][k])
        assert float((a[1] - b[1]).abs().max()) <= 1e-7 * float(b[1].abs().max()) + 1e-9

    host_aug = PN.apply_batch(u8, progs.chains)
    assert not np.array_equal(host_aug, u8)
    dev_aug = ops.photo_augment_u8(ctx, torch.from_numpy(u8).cuda(), progs).cpu().numpy()
    assert np.array_equal(dev_aug, host_aug)
    base = step(u8, None)
    same(step(u8, progs), step(host_aug, None))
    same(step(u8, None), base)
    assert abs(step(u8, progs)[0]["total"] - base[0]["total"]) > 1e-4  # (the chain did change the step)
    same(step(u8, progs, look_ahead=True), step(host_aug, None, look_ahead=True))


def test_forward_u8_with_photometric_programs(ctx):
    """forward_u8(photometric=P): the stem's input is that of the host-restated images, byte for byte; photometric=None: that
    of the batch as it is"""
    from pyrapose_amd import arch
    from pyrapose_amd.engine import Engine
    from pyrapose_amd.utils import photometric as PH
    B, H, W, C = 2, 64, 96, 5
    u8 = _images(8, B, H, W)
    rng = np.random.default_rng(12)
    progs = PH.compile_chain([PH.sample_chain(rng) + [PH.op_gray(0.1)] for _ in range(B)])
    eng = Engine(ctx, C, B, H, W, weights=arch.init_weights(C, seed=1), train=True)

    def stem_input(img, photometric):
        eng.forward_u8(torch.from_numpy(img).cuda(), photometric=photometric)
        torch.cuda.synchronize()
        return eng.acts["input4"].t.clone()
    a, b, c = stem_input(u8, progs), stem_input(PN.apply_batch(u8, progs.chains), None), stem_input(u8, None)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    eng.close()
