"""float64 numpy restatement of csrc/wpnp.hip: pp_vote_stats_f64 (votes -> per-corner mean, covariance and the 2x2 weight)
and pp_pnp_refine_weighted_f64 (the weighted reprojection cost of uncertainty_pnp/src/uncertainty_pnp.cpp:17-33 minimised
by this library's Levenberg-Marquardt).  Same rules, same order of the decisions; sums are numpy's, not the kernel's
fixed-order trees, so the two agree to rounding, not bitwise.  The GPU tests compare the device with this file."""
import numpy as np

FULL, ISO = 0, 1
CONVERGED, MAX_ITER, TOO_FEW, SINGULAR, BEHIND = 0, 1, 2, 3, 4
LM_DIAG_MIN, LM_DIAG_MAX, LM_LAMBDA0, LM_MIN_RHO = 1e-6, 1e32, 1e-4, 1e-3
LM_LAMBDA_MIN, LM_LAMBDA_MAX = 1e-16, 1e32


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def so3_coeffs(th):
    """a = sin(th)/th, b = (1-cos th)/th^2, c = (th - sin th)/th^3, by their series below 1e-4"""
    if th < 1e-4:
        t2 = th * th
        return 1.0 - t2 / 6.0, 0.5 - t2 / 24.0, 1.0 / 6.0 - t2 / 120.0
    return np.sin(th) / th, (1.0 - np.cos(th)) / (th * th), (th - np.sin(th)) / (th * th * th)


def rodrigues(w):
    w = np.asarray(w, np.float64)
    a, b, _ = so3_coeffs(float(np.sqrt(w @ w)))
    Kx = skew(w)
    return np.eye(3) + a * Kx + b * (Kx @ Kx)


def left_jacobian(w):
    """d(R(w) X)/dw = -[R X]x Jl(w)"""
    w = np.asarray(w, np.float64)
    _, b, c = so3_coeffs(float(np.sqrt(w @ w)))
    Kx = skew(w)
    return np.eye(3) + b * Kx + c * (Kx @ Kx)


def so3_log(R):
    R = np.asarray(R, np.float64)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = 0.5 * float(np.sqrt(v @ v))
    c = 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0)
    th = float(np.arctan2(s, c))
    if s < 1e-6 and c < 0.0:  # near pi: the axis from the symmetric part, signed by v
        A = 0.5 * (R + np.eye(3))
        d = np.sqrt(np.maximum(np.diag(A), 0.0))
        k = int(np.argmax(d))
        ax = A[:, k] / max(d[k], 1e-300)
        if float(v @ ax) < 0.0:
            ax = -ax
        return th * ax / float(np.sqrt(ax @ ax))
    if s < 1e-12:
        return 0.5 * v
    return (th / (2.0 * s)) * v


def residuals(x, obj, img, wgt, K4):
    """[n,2] weighted residuals, and z [n]"""
    R, t = rodrigues(x[:3]), x[3:]
    p = obj @ R.T + t
    dx = K4[0] * p[:, 0] / p[:, 2] + K4[2] - img[:, 0]
    dy = K4[1] * p[:, 1] / p[:, 2] + K4[3] - img[:, 1]
    return np.stack([wgt[:, 0] * dx + wgt[:, 1] * dy, wgt[:, 1] * dx + wgt[:, 2] * dy], 1), p[:, 2]


def jacobian(x, obj, img, wgt, K4):
    """analytic [n,2,6] Jacobian of residuals() in (w, t)"""
    R, t = rodrigues(x[:3]), x[3:]
    Jl = left_jacobian(x[:3])
    q = obj @ R.T
    p = q + t
    z = p[:, 2]
    ju0, ju2 = K4[0] / z, -K4[0] * p[:, 0] / (z * z)
    jv1, jv2 = K4[1] / z, -K4[1] * p[:, 1] / (z * z)
    zero = np.zeros_like(z)
    # rows of d(u, v)/d(phi) for a left perturbation exp(phi) R: d p / d phi = -[q]x
    Lu = np.stack([ju2 * q[:, 1], ju0 * q[:, 2] - ju2 * q[:, 0], -ju0 * q[:, 1]], 1)
    Lv = np.stack([jv2 * q[:, 1] - jv1 * q[:, 2], -jv2 * q[:, 0], jv1 * q[:, 0]], 1)
    Ju = np.concatenate([Lu @ Jl, np.stack([ju0, zero, ju2], 1)], 1)
    Jv = np.concatenate([Lv @ Jl, np.stack([zero, jv1, jv2], 1)], 1)
    J0 = wgt[:, 0:1] * Ju + wgt[:, 1:2] * Jv
    J1 = wgt[:, 1:2] * Ju + wgt[:, 2:3] * Jv
    return np.stack([J0, J1], 1)


def evaluate(x, obj, img, wgt, K4):
    """one pass: cost, J^T J, J^T r, points behind the camera, over the correspondences with a non-zero weight"""
    live = (wgt != 0.0).any(1)
    obj, img, wgt = obj[live], img[live], wgt[live]
    r, z = residuals(x, obj, img, wgt, K4)
    behind = int((~(z > 0.0)).sum())
    if behind:
        return np.inf, None, None, behind
    J = jacobian(x, obj, img, wgt, K4).reshape(-1, 6)
    r = r.reshape(-1)
    return 0.5 * float(r @ r), J.T @ J, J.T @ r, 0


def ldlt_solve(A, b):
    """LDL^T without pivoting; None when a pivot is not positive and finite"""
    n = len(b)
    L, D = np.eye(n), np.zeros(n)
    for j in range(n):
        d = A[j, j] - float((L[j, :j] ** 2) @ D[:j])
        if not (d > 0.0 and d < np.inf):
            return None
        D[j] = d
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - float((L[i, :j] * L[j, :j]) @ D[:j])) / d
    y = np.zeros(n)
    for i in range(n):
        y[i] = b[i] - float(L[i, :i] @ y[:i])
    y /= D
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = y[i] - float(L[i + 1:, i] @ x[i + 1:])
    return x


def pose_covariance(H):
    out = np.zeros((6, 6))
    for k in range(6):
        e = np.zeros(6)
        e[k] = 1.0
        col = ldlt_solve(H, e)
        if col is None:
            return np.zeros((6, 6))
        out[:, k] = col
    return out


def refine_weighted(obj, img, wgt, K4, R_init, t_init, max_iterations=50, gradient_tol=1e-10, parameter_tol=1e-8, function_tol=1e-6):
    """-> dict(R, t, rvec, cost_init, cost_final, iterations, status, pose_cov, trace).  trace: one (test name, value,
    threshold) per stopping test evaluated, in order."""
    obj = np.asarray(obj, np.float64).reshape(-1, 3)
    img = np.asarray(img, np.float64).reshape(-1, 2)
    wgt = np.asarray(wgt, np.float64).reshape(-1, 3)
    K4 = np.asarray(K4, np.float64).reshape(4)
    R_init, t_init = np.asarray(R_init, np.float64).reshape(3, 3), np.asarray(t_init, np.float64).reshape(3)
    x = np.concatenate([so3_log(R_init), t_init])
    trace = []

    def fail(status, passes, cost=0.0):
        return dict(R=R_init.copy(), t=t_init.copy(), rvec=x[:3].copy(), cost_init=cost, cost_final=cost, iterations=passes,
                    status=status, pose_cov=np.zeros((6, 6)), trace=trace)

    if int((wgt != 0.0).any(1).sum()) < 3:
        return fail(TOO_FEW, 0)
    cost, H, g, behind = evaluate(x, obj, img, wgt, K4)
    passes = 1
    if behind:
        return fail(BEHIND, passes)
    if not np.isfinite(cost):
        return fail(SINGULAR, passes)
    cost_init = cost
    lam, nu = LM_LAMBDA0, 2.0
    status = None
    gmax = float(np.abs(g).max())
    trace.append(("gradient", gmax, gradient_tol))
    if gmax < gradient_tol:
        status = CONVERGED
    while status is None:
        if passes - 1 >= max_iterations:
            status = MAX_ITER
            break
        D = np.clip(np.diag(H), LM_DIAG_MIN, LM_DIAG_MAX)
        delta = ldlt_solve(H + lam * np.diag(D), -g)
        if delta is None or not np.isfinite(delta).all():
            return fail(SINGULAR, passes, cost_init)
        step, xn = float(np.sqrt(delta @ delta)), float(np.sqrt(x @ x))
        trace.append(("parameter", step, parameter_tol * (xn + parameter_tol)))
        if step <= parameter_tol * (xn + parameter_tol):
            status = CONVERGED
            break
        pred = -float(g @ delta) - 0.5 * float(delta @ (H @ delta))
        x_new = x + delta
        cost_new, H_new, g_new, behind = evaluate(x_new, obj, img, wgt, K4)
        passes += 1
        rho = -1.0
        if not behind and np.isfinite(cost_new) and pred > 0.0:
            rho = (cost - cost_new) / pred
        if rho > LM_MIN_RHO:
            dcost, cost_old = cost - cost_new, cost
            x, cost, H, g = x_new, cost_new, H_new, g_new
            lam = min(max(lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), LM_LAMBDA_MIN), LM_LAMBDA_MAX)
            nu = 2.0
            gmax = float(np.abs(g).max())
            trace.append(("gradient", gmax, gradient_tol))
            if gmax < gradient_tol:
                status = CONVERGED
                break
            trace.append(("function", dcost, function_tol * cost_old))
            if dcost <= function_tol * cost_old:
                status = CONVERGED
                break
        else:
            lam = min(lam * nu, LM_LAMBDA_MAX)
            nu = 2.0 * nu
    return dict(R=rodrigues(x[:3]), t=x[3:].copy(), rvec=x[:3].copy(), cost_init=cost_init, cost_final=cost, iterations=passes,
                status=status, pose_cov=pose_covariance(H), trace=trace)


def trace_is_clear(trace, factor=10.0):
    """no stopping test of the trace came within `factor` of its threshold (either side)"""
    for _name, value, thr in trace:
        if thr > 0.0 and thr / factor <= value <= thr * factor:
            return False
    return True


def weight_from_cov(cov3, n_eff, mode, sigma_floor):
    """cov3 = (xx, xy, yy) -> (wxx, wxy, wyy)"""
    if mode == ISO:
        if cov3[0] < 1e-5:
            return np.zeros(3)
        m, d = 0.5 * (cov3[0] + cov3[2]), 0.5 * (cov3[0] - cov3[2])
        w = 1.0 / (m + np.sqrt(d * d + cov3[1] * cov3[1]))
        return np.array([w, 0.0, w])
    s2 = sigma_floor * sigma_floor
    a, b, c = cov3[0] / n_eff + s2, cov3[1] / n_eff, cov3[2] / n_eff + s2
    m, d = 0.5 * (a + c), 0.5 * (a - c)
    r = np.sqrt(d * d + b * b)
    l1, l2 = m + r, m - r
    if not (l2 > 0.0):
        return np.zeros(3)
    f1, f2 = 1.0 / np.sqrt(l1), 1.0 / np.sqrt(l2)
    if r == 0.0:
        return np.array([f1, 0.0, f1])
    # W = f2 I + (f1 - f2) P1, P1 = (C - l2 I) / (2 r) the projector on the major axis
    k = (f1 - f2) / (2.0 * r)
    return np.array([f2 + k * (d + r), k * b, f2 + k * (r - d)])


def vote_stats(img, offsets, ppv=8, vote_weight=None, inlier_mask=None, mode=FULL, sigma_floor=0.5):
    """-> dict(wsum [P,ppv], count [P,ppv], mu [P,ppv,2], cov [P,ppv,3], n_eff [P,ppv], wgt [P,ppv,3])"""
    img = np.asarray(img, np.float64).reshape(-1, 2)
    offsets = np.asarray(offsets)
    P = len(offsets) - 1
    out = dict(wsum=np.zeros((P, ppv)), count=np.zeros((P, ppv), np.int32), mu=np.zeros((P, ppv, 2)), cov=np.zeros((P, ppv, 3)),
               n_eff=np.zeros((P, ppv)), wgt=np.zeros((P, ppv, 3)))
    for p in range(P):
        p0, n = int(offsets[p]), int(offsets[p + 1] - offsets[p])
        k = n // ppv
        w_all = np.ones(k) if vote_weight is None else np.asarray(vote_weight, np.float64)[p0 // ppv: p0 // ppv + k]
        for j in range(ppv):
            idx = p0 + np.arange(k) * ppv + j
            w = w_all.copy()
            if inlier_mask is not None:
                w = np.where(np.asarray(inlier_mask)[idx] != 0, w, 0.0)
            w = np.where(w > 0.0, w, 0.0)
            cnt, ws = int((w > 0.0).sum()), float(w.sum())
            out["count"][p, j], out["wsum"][p, j] = cnt, ws
            if cnt < 1:
                continue
            xy = img[idx]
            mu = (w[:, None] * xy).sum(0) / ws
            c = xy - mu
            cov = np.array([(w * c[:, 0] * c[:, 0]).sum(), (w * c[:, 0] * c[:, 1]).sum(), (w * c[:, 1] * c[:, 1]).sum()]) / ws
            ne = ws * ws / float((w * w).sum())
            out["mu"][p, j], out["cov"][p, j], out["n_eff"][p, j] = mu, cov, ne
            if cnt >= 2:
                out["wgt"][p, j] = weight_from_cov(cov, ne, mode, sigma_floor)
    return out
