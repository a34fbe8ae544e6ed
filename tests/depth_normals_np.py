"""float64 numpy restatement of pp_depth_normals_f64 (csrc/depth_image.hip): the reference's get_normal
(annotation_scripts/Augmentations.py:394-467) with every operation in the order the device takes it, so that the device
outputs are these bits.  The Gaussian is its own loop with a fixed tap order (the first tap, then the others in increasing
index) over np.pad(..., mode='symmetric'), which is scipy's border mode 'reflect'; gradient, cross product, norm and the NaN
rule are numpy's own functions, as in the reference.  Two things are not the reference's: the degenerate-image rule (an
image whose largest smoothed depth, or largest scaled normal component, is 0 gives an all-zero uint8 image and scaled depth,
where the reference divides by zero), and the `signed` output (the unit normals before abs)."""
import numpy as np

RADIUS = 8  # int(4 * 2 + 0.5)


def gaussian_taps(sigma=2.0, truncate=4.0):
    """scipy.ndimage's _gaussian_kernel1d: exp(-x^2 / (2 sigma^2)) over -r..r, divided by its sum"""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return w / w.sum()


def _filter_axis0(a, w):
    r = (len(w) - 1) // 2
    p = np.pad(a, ((r, r), (0, 0)), mode="symmetric")
    n = a.shape[0]
    acc = w[0] * p[0:n]
    for k in range(1, len(w)):
        acc = acc + w[k] * p[k:k + n]
    return acc


def smooth(depth):
    """gaussian_filter(depth, 2) in float64: axis 0, then axis 1"""
    w = gaussian_taps(2.0)
    d = _filter_axis0(np.asarray(depth, np.float64), w)
    return np.ascontiguousarray(_filter_axis0(d.T, w).T)


def depth_normals(depth, fx, cx, cy, for_vis=True):
    """depth [H,W] -> dict: 'normals' float64 [H,W,3], 'signed' float64 [H,W,3], 'depth' float64 [H,W] (scaled by 1 / its
    maximum when for_vis is False) and, when for_vis is False, 'normals_u8' uint8 [H,W,3]"""
    depth = np.asarray(depth)
    H, W = depth.shape
    d = smooth(depth)
    c = 1.0 / np.float64(fx)
    u = np.zeros(W, np.int16)
    v = np.zeros(H, np.int16)
    u[:] = np.arange(0, W) - np.float64(cx)  # the assignment truncates toward zero
    v[:] = np.arange(0, H) - np.float64(cy)
    u = np.broadcast_to(u[None, :], (H, W))
    v = np.broadcast_to(v[:, None], (H, W))
    gy, gx = np.gradient(d, 2, edge_order=2)
    v_x = np.zeros((H, W, 3))
    v_y = np.zeros((H, W, 3))
    v_y[:, :, 0] = u * c * gy
    v_y[:, :, 1] = d * c + (v * c) * gy
    v_y[:, :, 2] = gy
    v_x[:, :, 0] = d * c + u * c * gx
    v_x[:, :, 1] = v * c * gx
    v_x[:, :, 2] = gx
    with np.errstate(invalid="ignore", divide="ignore"):
        cross = np.cross(v_x.reshape(-1, 3), v_y.reshape(-1, 3))
        norm = np.expand_dims(np.linalg.norm(cross, axis=1), axis=1)
        signed = np.nan_to_num((cross / norm).reshape(H, W, 3))
    signed[d > 2000] = 0
    n = np.abs(signed)
    out = {"normals": n, "signed": signed, "depth": d}
    if for_vis:
        return out
    dmax = np.max(d)
    m = None
    if dmax > 0:
        ds = d * (1.0 / dmax)
        m = n * (1 - (ds - 0.5))[:, :, None]
    if m is None or np.max(m) == 0:  # the degenerate image
        out["depth"] = np.zeros((H, W), np.float64)
        out["normals_u8"] = np.zeros((H, W, 3), np.uint8)
        return out
    out["depth"] = ds
    out["normals_u8"] = (m * (255.0 / np.max(m))).astype(np.uint8)
    return out


def depth_normals_batch(depth, intr, for_vis=True):
    """depth [n,H,W], intr [n,3] = (fx, cx, cy) -> the same dict with a leading n"""
    outs = [depth_normals(dep, *[float(x) for x in k], for_vis=for_vis) for dep, k in zip(depth, intr)]
    return {key: np.stack([o[key] for o in outs]) for key in outs[0]}
