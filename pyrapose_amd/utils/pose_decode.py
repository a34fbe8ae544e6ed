"""From the prediction model's outputs to object poses: the per-image, per-class block of the evaluation loops
(utils/linemod_eval.py:303-333 threshold + vote count, :421-431 correspondences, :479-485 PnP), batched on the device.

    for inv_cls in range(scores.shape[2]):
        cls_indices = np.where(scores[0, :, inv_cls] > threshold)        # ascending anchor order (D3)
        if len(cls_indices[0]) < 10: continue                            # < 1 in occlusion_eval.py:359-371
        est_points = boxes3D[0, cls_indices, :].reshape(k * 8, 1, 2);  obj_points = repeat(threeD_boxes[cls], k)
        retval, rvec, tvec, inliers = cv2.solvePnPRansac(obj_points, est_points, K, None, 300, 5.0, 0.99, ITERATIVE)
"""
from types import SimpleNamespace

import numpy as np
import torch

from .. import ops
from ..runtime import default_context
from ._host import k4, to_device


def _problems_per_class(idx, cnt, min_votes):
    """One problem per (image, class) with at least min_votes votes, (b, c) ascending; None when there is none.  The record:
    pb / pc (/ pk: instance, here None) per problem, b_of / c_of / anchor per vote in problem order, k votes per problem."""
    sel = cnt >= min_votes                                                     # [B, C]
    if not bool(sel.any()):
        return None
    # everything stays on the device until the poses come back: one gather for all (image, class) problems
    live = (torch.arange(idx.shape[2], device="cuda")[None, None, :] < cnt[:, :, None]) & sel[:, :, None]  # [B, C, cap], (b, c, vote) order
    b_of, c_of, _ = torch.nonzero(live, as_tuple=True)
    pb, pc = torch.nonzero(sel, as_tuple=True)
    return SimpleNamespace(pb=pb, pc=pc, pk=None, b_of=b_of, c_of=c_of, anchor=idx[live].long(), k=cnt[sel].long())


def _problems_per_instance(ctx, boxes3D, scores, idx, cnt, min_votes, instances):
    """One problem per (image, class, instance) of ops.vote_cluster, ascending; None when there is none.  The record of
    _problems_per_class with pk set, plus lead / lbox: each problem's leader anchor and its vote box."""
    mi = int(instances.get("max_instances", 8))
    _inst, order, ioffs, n_inst, lead, lbox = ops.vote_cluster(ctx, boxes3D, scores, idx, cnt, float(instances.get("iou", 0.5)), min_votes, mi,
                                                               instances.get("max_rounds"))
    sel = torch.arange(mi, device="cuda")[None, None, :] < n_inst[:, :, None]  # [B, C, max_instances]
    if not bool(sel.any()):
        return None
    # `order` already lists the kept votes instance-major, so the same gather over its first inst_offsets[.., -1] entries
    # yields the votes in problem order
    live = torch.arange(idx.shape[2], device="cuda")[None, None, :] < ioffs[:, :, mi:]
    b_of, c_of, _ = torch.nonzero(live, as_tuple=True)
    pb, pc, pk = torch.nonzero(sel, as_tuple=True)
    return SimpleNamespace(pb=pb, pc=pc, pk=pk, b_of=b_of, c_of=c_of, anchor=order[live].long(),
                           k=(ioffs[:, :, 1:] - ioffs[:, :, :-1])[sel].long(), lead=lead[sel], lbox=lbox[sel])


def _weighted(ctx, pr, ransac, weighting, scores, corners, sigma_floor):
    """The weighted stage on the RANSAC poses of the problems `pr` (with offs / obj / img / K_p set): (R, t, extra), a problem
    whose RANSAC failed or whose refinement did not end converged / at max_iterations keeping its RANSAC pose."""
    R, t, mask, ok = ransac
    score = scores[pr.b_of, pr.anchor, pr.c_of].double().contiguous()          # one per vote, (b, c, vote) order
    if weighting == "corners":
        st = ops.vote_stats(ctx, pr.offs, pr.img, 8, score, mask, "full", float(sigma_floor), check_offsets=False)
        o8 = (8 * torch.arange(int(pr.k.numel()) + 1, device="cuda")).to(torch.int32)
        ref = ops.pnp_refine_weighted(ctx, o8, corners[pr.pc].reshape(-1, 3).contiguous(), st["mu"].reshape(-1, 2), st["wgt"].reshape(-1, 3),
                                      pr.K_p, R, t, check_offsets=False)
    else:
        w = score.repeat_interleave(8) * mask.double()
        wgt = torch.stack([w, torch.zeros_like(w), w], 1).contiguous()
        ref = ops.pnp_refine_weighted(ctx, pr.offs, pr.obj, pr.img, wgt, pr.K_p, R, t, check_offsets=False)
    use = (ok != 0) & (ref["status"] <= ops.WPNP_MAX_ITER)
    extra = dict(R_ransac=R.cpu().numpy(), t_ransac=t.cpu().numpy(), cost=torch.where(use, ref["cost_final"], ref["cost_init"]).cpu().numpy(),
                 cost_ransac=ref["cost_init"].cpu().numpy(), pose_cov=ref["pose_cov"].cpu().numpy(), refine_status=ref["status"].cpu().numpy())
    return torch.where(use[:, None, None], ref["R"], R), torch.where(use[:, None], ref["t"], t), extra


def _to_dicts(pr, R, t, mask, ok, extra, scores):
    """the output list of poses_from_outputs, one dict per problem in problem order"""
    R, t, mask, ok = R.cpu().numpy(), t.cpu().numpy(), mask.cpu().numpy(), ok.cpu().numpy()
    offs, anchor, k = pr.offs.cpu().numpy(), pr.anchor.cpu().numpy(), pr.k.cpu().numpy()
    if pr.pk is not None:
        pk, lead, lbox, lscore = pr.pk.cpu().numpy(), pr.lead.cpu().numpy(), pr.lbox.cpu().numpy(), scores[pr.pb, pr.lead.long(), pr.pc].cpu().numpy()
    pb, pc = pr.pb.cpu().numpy(), pr.pc.cpu().numpy()
    out, v0 = [], 0
    for p in range(len(k)):
        d = dict(image=int(pb[p]), cls=int(pc[p]), votes=anchor[v0: v0 + k[p]], ok=bool(ok[p]), R=R[p], t=t[p],
                 inliers=np.nonzero(mask[offs[p]:offs[p + 1]])[0])
        if extra is not None:
            d.update(R_ransac=extra["R_ransac"][p], t_ransac=extra["t_ransac"][p], cost=float(extra["cost"][p]),
                     cost_ransac=float(extra["cost_ransac"][p]), pose_cov=extra["pose_cov"][p], refine_status=int(extra["refine_status"][p]))
        if pr.pk is not None:
            d.update(instance=int(pk[p]), leader=int(lead[p]), box=lbox[p], score=float(lscore[p]))
        out.append(d)
        v0 += int(k[p])
    return out


def poses_from_outputs(boxes3D, scores, threeD_boxes, K, threshold=0.5, min_votes=10, iterations=300, reproj_error=5.0, seed=0,
                       ctx=None, weighting=None, sigma_floor=0.5, instances=None):
    """boxes3D [B,N,16], scores [B,N,C] (numpy or cuda float32 tensors: predict_on_batch outputs); threeD_boxes [C,8,3]
    cuboid corners per class (model units); K 3x3 or [B,3,3].  Returns one dict per (image, class) that reached
    `min_votes` votes, image-major then class ascending like the reference loop:
    {image, cls (0-based), votes (ascending anchor indices), ok, R [3,3], t [3], inliers (indices into votes x 8 corners)}.

    weighting: None (the RANSAC pose, as above), or an uncertainty-weighted refinement of it on the device (csrc/wpnp.hip; the
    call the reference prepares at linemod_eval.py:488-496):
      'corners': per corner the score-weighted mean of the RANSAC-inlier votes and W = (cov / n_eff + sigma_floor^2 I)^(-1/2)
                 (ops.vote_stats), then the solver on the 8 (corner, mean, W) correspondences;
      'scores':  every inlier vote stays a correspondence with wxx = wyy = its class score, wxy = 0 (pose_weights there).
    The dicts then gain R_ransac, t_ransac, cost (of the returned pose), cost_ransac (of the RANSAC pose under the same
    weights), pose_cov [6,6] and refine_status (ops.WPNP_*); a problem whose RANSAC failed or whose refinement did not end
    converged / at max_iterations keeps the RANSAC pose.

    instances: None (one problem per (image, class), the reference's one-object-per-class assumption, tless_eval.py:378), or a
    dict with any of iou (0.5), max_instances (8), max_rounds (4 * max_instances): the votes of each (image, class) are first
    clustered into object instances by vote-box IoU (ops.vote_cluster -- the library's own step, no counterpart in the
    reference) and every instance is its own problem, enumerated (image, class, instance) ascending; `min_votes` then applies
    per instance and `weighting` per problem as before.  Each dict gains instance, leader (anchor index of the cluster's
    best-scored vote), box (its vote box x1, y1, x2, y2 in pixels) and score (its class score)."""
    if weighting not in (None, "corners", "scores"):
        raise ValueError("weighting must be None, 'corners' or 'scores'")
    if instances is not None and (not isinstance(instances, dict) or set(instances) - {"iou", "max_instances", "max_rounds"}):
        raise ValueError("instances must be None or a dict with iou / max_instances / max_rounds")
    ctx = ctx or default_context()
    boxes3D, scores = to_device(boxes3D, torch.float32), to_device(scores, torch.float32)
    B, N, C = scores.shape
    corners = to_device(threeD_boxes, shape=(C, 8, 3))
    K_all = to_device(k4(K, B))  # K 3x3 or [B,3,3], anything else is a ValueError
    idx, cnt = ops.score_threshold_compact(ctx, scores, float(threshold))  # bit-exact np.where order
    mv = max(int(min_votes), 1)
    pr = _problems_per_class(idx, cnt, mv) if instances is None else _problems_per_instance(ctx, boxes3D, scores, idx, cnt, mv, instances)
    if pr is None:
        return []
    pr.img = boxes3D[pr.b_of, pr.anchor, :].double().reshape(-1, 2).contiguous()
    pr.obj = corners[pr.c_of].reshape(-1, 3).contiguous()
    pr.offs = torch.zeros((pr.k.numel() + 1,), dtype=torch.int32, device="cuda")
    pr.offs[1:] = (8 * torch.cumsum(pr.k, 0)).to(torch.int32)
    pr.K_p = K_all[pr.pb].contiguous()
    R, t, _n_in, mask, ok = ops.pnp_ransac(ctx, pr.offs, pr.obj, pr.img, pr.K_p, iterations, reproj_error, seed, 8)
    extra = None
    if weighting is not None:
        R, t, extra = _weighted(ctx, pr, (R, t, mask, ok), weighting, scores, corners, sigma_floor)
    return _to_dicts(pr, R, t, mask, ok, extra, scores)
