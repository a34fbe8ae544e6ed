"""numpy restatement of the scene ground-truth pass (pp_scene_gt_info, csrc/scene_gt.hip), pixel by pixel in the same expression
order: from a stack of instance depth images grouped into scenes, the composed scene depth, the three pixel counts, both boxes
and both masks of every instance (bop_toolkit's calc_gt_info / calc_gt_masks, definitions restated) and the id image
(annotate_BOP.py:363-374: instances in order, later ones overwrite earlier ones).  The distance images and the 'bop19'
visibility test are those of tests/vsd_bop_np.py."""
import numpy as np

from tests.vsd_bop_np import dist_im, visib_mask


def compose_depth(stack):
    """[m,h,w] -> per pixel the smallest positive depth, 0 where there is none (float32)"""
    stack = np.asarray(stack, np.float32)
    out = np.zeros(stack.shape[1:], np.float32)
    for d in stack:
        take = (d > 0) & ((out == 0) | (d < out))
        out = np.where(take, d, out)
    return out


def box(mask, off_x=0, off_y=0):
    """(x, y, w, h) of a non-empty bool mask, w = x_max - x_min, h = y_max - y_min, moved by the window's offset"""
    rows, cols = np.nonzero(mask)
    return [int(cols.min()) - off_x, int(rows.min()) - off_y, int(cols.max() - cols.min()), int(rows.max() - rows.min())]


def scene_gt(stack, scene_offsets, K, depth_test=None, delta=15.0, window=None):
    """stack float32 [n,ch,cw], scene_offsets [S+1], K 3x3 (image coordinates) or [n,3,3], depth_test None, [h,w] or [S,h,w],
    window (off_x, off_y, w, h) or None -> dict: px_count int64 [n,3] (all, valid, visib), bbox_obj, bbox_visib int32 [n,4],
    id_image uint8 [S,h,w], scene_depth float32 [S,h,w] (None with depth_test), mask_full, mask_visib uint8 [n,h,w]"""
    stack = np.asarray(stack, np.float32)
    n, ch, cw = stack.shape
    S = len(scene_offsets) - 1
    off_x, off_y, w, h = window if window is not None else (0, 0, cw, ch)
    K = np.asarray(K, np.float64)
    Ks = np.broadcast_to(K, (n, 3, 3)) if K.ndim == 2 else K
    inside = stack[:, off_y:off_y + h, off_x:off_x + w]
    composed = None
    if depth_test is None:
        composed = np.stack([compose_depth(inside[scene_offsets[s]:scene_offsets[s + 1]]) for s in range(S)])
        tests = composed
    else:
        depth_test = np.asarray(depth_test, np.float32)
        tests = np.broadcast_to(depth_test, (S, h, w)) if depth_test.ndim == 2 else depth_test
    px_count = np.zeros((n, 3), np.int64)
    bbox_obj, bbox_visib = np.full((n, 4), -1, np.int32), np.full((n, 4), -1, np.int32)
    mask_full, mask_visib = np.zeros((n, h, w), np.uint8), np.zeros((n, h, w), np.uint8)
    id_image = np.zeros((S, h, w), np.uint8)
    for s in range(S):
        for i in range(scene_offsets[s], scene_offsets[s + 1]):
            d_gt, d_test = inside[i], tests[s]
            vis = visib_mask(dist_im(d_test, Ks[i]), dist_im(d_gt, Ks[i]), delta, "bop19")
            px_count[i] = [(stack[i] > 0).sum(), ((d_gt > 0) & (d_test > 0)).sum(), vis.sum()]
            mask_full[i] = np.where(d_gt > 0, 255, 0)
            mask_visib[i] = np.where(vis, 255, 0)
            if vis.any():
                bbox_obj[i] = box(stack[i] > 0, off_x, off_y)
                bbox_visib[i] = box(vis)
            id_image[s] = np.where(vis, i - scene_offsets[s] + 1, id_image[s])
    return dict(px_count=px_count, bbox_obj=bbox_obj, bbox_visib=bbox_visib, id_image=id_image, scene_depth=composed,
                mask_full=mask_full, mask_visib=mask_visib)
