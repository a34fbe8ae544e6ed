// Uncertainty-weighted PnP refinement of voted poses: the reference's uncertainty_pnp/ (a Ceres problem,
// src/uncertainty_pnp.cpp:7-92, wrapped by un_pnp_utils.py and prepared at utils/linemod_eval.py:488-496), batched on the
// device.  Ceres is third-party and absent: PARITY WITH CERES UNPINNED.  What is pinned is the cost function (the functor of
// uncertainty_pnp.cpp:17-33) and its minimum; the minimiser is this library's own, restated in tests/wpnp_np.py.
//
// pp_vote_stats_f64: votes -> per-corner statistics.  One workgroup per problem, one wave per corner (corners wave, wave + 4,
//   ...), lanes stride over the votes; two passes (weighted mean, then centred second moments), wave all-reduce by xor
//   butterflies (commutative additions: every lane holds the same bits).  Weight modes: PP_WPNP_FULL
//   W = (cov / n_eff + sigma_floor^2 I)^(-1/2) by the closed-form 2x2 eigen-decomposition (W = f2 I + (f1 - f2) P1, f = 1 /
//   sqrt(lambda), P1 the projector on the major axis; W = 0 when lambda_min <= 0); PP_WPNP_ISO w = 1 / lambda_max(cov),
//   0 where cov_xx < 1e-5 (un_pnp_utils.py:75-83, 103-104).  count < 2: W = 0.
//
// pp_pnp_refine_weighted_f64: parameters x = (w, t), w the angle-axis vector (taken from R_init by the kernel).  Per
//   correspondence with a non-zero weight: p = Rodrigues(w) X + t, d = (fx p_x / p_z + cx - u, fy p_y / p_z + cy - v),
//   r = (wxx d_x + wxy d_y, wxy d_x + wyy d_y), cost = 1/2 sum |r|^2; analytic Jacobian (d p / d w = -[R X]x Jl(w), Jl the left
//   Jacobian of SO(3)).  Levenberg-Marquardt:
//     pass 1 at the start: cost, H = J^T J, g = J^T r, the number of weighted points and of those with p_z <= 0
//       (fewer than 3 weighted: TOO_FEW, 0 passes; any behind: BEHIND; cost not finite: SINGULAR; max |g| < gradient_tol: CONVERGED);
//     loop, lambda = 1e-4, nu = 2:  passes - 1 >= max_iterations -> MAX_ITER;
//       D = clamp(diag H, 1e-6, 1e32); (H + lambda diag D) delta = -g by LDL^T (a pivot not in (0, inf), or a non-finite delta:
//       SINGULAR, the START pose is returned); |delta| <= parameter_tol (|x| + parameter_tol) -> CONVERGED;
//       pred = -g.delta - 1/2 delta^T H delta; ONE pass at x + delta gives the trial cost and the trial H, g together;
//       rho = (cost - cost_new) / pred, or -1 when a weighted point is behind the camera, the trial cost is not finite or pred <= 0;
//       rho > 1e-3: accept (x, cost, H, g <- trial), lambda <- clamp(lambda max(1/3, 1 - (2 rho - 1)^3), 1e-16, 1e32), nu <- 2,
//         then max |g| < gradient_tol -> CONVERGED, cost decrease <= function_tol * (cost before the step) -> CONVERGED;
//       else lambda <- min(lambda nu, 1e32), nu <- 2 nu.
//   Only accepted steps move the pose: cost_final <= cost_init exactly.  pose_cov = H^-1 at the final pose by LDL^T (zeros when a
//   pivot fails).  `iterations` = passes run.
// Two paths, chosen by the problem's OWN size (a result never depends on its batch): n <= 64 one wave64 per problem, four
// problems per workgroup, one correspondence per lane in registers, xor-butterfly all-reduce, no barrier; n > 64 one workgroup
// of 256 threads per problem, correspondences in registers when a thread owns at most four (n <= 1024), per-thread sums in
// index order, wave butterfly, then the four wave sums added in wave order from a double-buffered LDS array (one barrier per
// pass).  Every thread solves the 6x6 system from the same sums, so all branches are uniform.  float64, -ffp-contract=off:
// bitwise equal run to run and independent of the batch.
#include "pp_internal.h"

#define WPNP_THREADS 256
#define WPNP_WAVES (WPNP_THREADS / 64)
#define WPNP_WAVE_MAX 64
#define WPNP_NS 30  // 21 (lower triangle of H, row-major) + 6 (g) + cost + points behind + weighted points

struct WpnpArgs {
  int n_problems, n_total;
  const int* offsets;
  const double* obj;   // [N][3]
  const double* img;   // [N][2]
  const double* wgt;   // [N][3] wxx, wxy, wyy
  const double* K4;    // [P][4]
  const double* R_init;
  const double* t_init;
  int max_iterations;
  double gtol, ptol, ftol;
  double *R_out, *t_out, *rvec_out, *cost_init, *cost_final;
  int *iterations, *status;
  double* pose_cov;    // [P][36] or NULL
};

__device__ __forceinline__ void wpnp_coeffs(double th, double* a, double* b, double* c) {
  if (th < 1e-4) {
    const double t2 = th * th;
    *a = 1.0 - t2 / 6.0;
    *b = 0.5 - t2 / 24.0;
    *c = 1.0 / 6.0 - t2 / 120.0;
  } else {
    *a = sin(th) / th;
    *b = (1.0 - cos(th)) / (th * th);
    *c = (th - sin(th)) / (th * th * th);
  }
}

// R = I + a [w]x + b [w]x^2 ; Jl = I + b [w]x + c [w]x^2
__device__ void wpnp_rot_and_jl(const double* w, double* R, double* Jl) {
  const double th = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  double a, b, c;
  wpnp_coeffs(th, &a, &b, &c);
  const double Kx[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) {
      double k2 = 0.0;
      for (int k = 0; k < 3; ++k) k2 += Kx[3 * r + k] * Kx[3 * k + q];
      const double id = r == q ? 1.0 : 0.0;
      R[3 * r + q] = id + a * Kx[3 * r + q] + b * k2;
      Jl[3 * r + q] = id + b * Kx[3 * r + q] + c * k2;
    }
}

__device__ void wpnp_log(const double* R, double* w) {
  const double v[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const double s = 0.5 * sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  const double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
  const double th = atan2(s, c);
  if (s < 1e-6 && c < 0.0) {  // near pi: the axis from the symmetric part, signed by v
    const double A[9] = {0.5 * (R[0] + 1.0), 0.5 * R[1], 0.5 * R[2], 0.5 * R[3], 0.5 * (R[4] + 1.0), 0.5 * R[5],
                         0.5 * R[6], 0.5 * R[7], 0.5 * (R[8] + 1.0)};
    const double d[3] = {sqrt(fmax(A[0], 0.0)), sqrt(fmax(A[4], 0.0)), sqrt(fmax(A[8], 0.0))};
    int k = 0;
    if (d[1] > d[k]) k = 1;
    if (d[2] > d[k]) k = 2;
    const double dk = fmax(d[k], 1e-300);
    double ax[3] = {A[k] / dk, A[3 + k] / dk, A[6 + k] / dk};
    if ((v[0] * ax[0] + v[1] * ax[1]) + v[2] * ax[2] < 0.0)
      for (int i = 0; i < 3; ++i) ax[i] = -ax[i];
    const double nn = sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]);
    for (int i = 0; i < 3; ++i) w[i] = th * ax[i] / nn;
    return;
  }
  const double f = s < 1e-12 ? 0.5 : th / (2.0 * s);
  for (int i = 0; i < 3; ++i) w[i] = f * v[i];
}

// one correspondence into the 30 running sums
__device__ __forceinline__ void wpnp_point(const double* R, const double* t, const double* Jl, double fx, double fy, double cx, double cy,
                                           const double* X, const double* uv, const double* wg, double* v) {
  const double wxx = wg[0], wxy = wg[1], wyy = wg[2];
  if (wxx == 0.0 && wxy == 0.0 && wyy == 0.0) return;
  v[29] += 1.0;
  const double qa = (X[0] * R[0] + X[1] * R[1]) + X[2] * R[2];
  const double qb = (X[0] * R[3] + X[1] * R[4]) + X[2] * R[5];
  const double qc = (X[0] * R[6] + X[1] * R[7]) + X[2] * R[8];
  const double x = qa + t[0], y = qb + t[1], z = qc + t[2];
  if (!(z > 0.0)) {
    v[28] += 1.0;
    return;
  }
  const double dx = fx * x / z + cx - uv[0], dy = fy * y / z + cy - uv[1];
  const double r0 = wxx * dx + wxy * dy, r1 = wxy * dx + wyy * dy;
  const double ju0 = fx / z, ju2 = -fx * x / (z * z), jv1 = fy / z, jv2 = -fy * y / (z * z);
  // rows of d(u, v) / d(phi) for a left perturbation exp(phi) R (d p / d phi = -[R X]x), then times Jl for d / d w
  const double Lu[3] = {ju2 * qb, ju0 * qc - ju2 * qa, -ju0 * qb};
  const double Lv[3] = {jv2 * qb - jv1 * qc, -jv2 * qa, jv1 * qa};
  double Ju[6], Jv[6];
  for (int c = 0; c < 3; ++c) {
    Ju[c] = (Lu[0] * Jl[c] + Lu[1] * Jl[3 + c]) + Lu[2] * Jl[6 + c];
    Jv[c] = (Lv[0] * Jl[c] + Lv[1] * Jl[3 + c]) + Lv[2] * Jl[6 + c];
  }
  Ju[3] = ju0; Ju[4] = 0.0; Ju[5] = ju2;
  Jv[3] = 0.0; Jv[4] = jv1; Jv[5] = jv2;
  double J0[6], J1[6];
  for (int k = 0; k < 6; ++k) {
    J0[k] = wxx * Ju[k] + wxy * Jv[k];
    J1[k] = wxy * Ju[k] + wyy * Jv[k];
  }
  int q = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c <= r; ++c, ++q) v[q] += J0[r] * J0[c] + J1[r] * J1[c];
  for (int r = 0; r < 6; ++r) v[21 + r] += J0[r] * r0 + J1[r] * r1;
  v[27] += 0.5 * (r0 * r0 + r1 * r1);
}

// LDL^T of a symmetric 6x6; false when a pivot is not positive and finite
__device__ bool wpnp_ldlt(const double (*A)[6], double (*L)[6], double* D) {
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k] * D[k];
    if (!(d > 0.0 && d < __longlong_as_double(0x7ff0000000000000ll))) return false;
    D[j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i][j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k] * D[k];
      L[i][j] = s / d;
    }
  }
  return true;
}

__device__ void wpnp_ldlt_solve(const double (*L)[6], const double* D, const double* b, double* x) {
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double s = b[i];
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s;
  }
  for (int i = 0; i < 6; ++i) y[i] = y[i] / D[i];
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
    for (int k = i + 1; k < 6; ++k) s -= L[k][i] * x[k];
    x[i] = s;
  }
}

__device__ __forceinline__ double wpnp_wave_allsum(double x) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

__device__ __forceinline__ bool wpnp_finite(double x) { return fabs(x) < __longlong_as_double(0x7ff0000000000000ll); }

// WAVE: one wave per problem (n <= 64).  !WAVE: one workgroup per problem; red = double-buffered [2][WPNP_WAVES][WPNP_NS]
template <bool WAVE>
__device__ void wpnp_problem(const WpnpArgs& a, int prob, int p0, int n, double* red) {
  constexpr int STRIDE = WAVE ? 64 : WPNP_THREADS;
  constexpr int NC = WAVE ? 1 : 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int id = WAVE ? lane : (int)threadIdx.x;
  const double* obj = a.obj + 3 * (size_t)p0;
  const double* img = a.img + 2 * (size_t)p0;
  const double* wgt = a.wgt + 3 * (size_t)p0;
  const double fx = a.K4[4 * prob], fy = a.K4[4 * prob + 1], cx = a.K4[4 * prob + 2], cy = a.K4[4 * prob + 3];
  const bool cached = n <= NC * STRIDE;
  double cX[NC][3], cU[NC][2], cW[NC][3];
  if (cached) {
    for (int c = 0; c < NC; ++c) {
      const int i = id + c * STRIDE;
      const bool in = i < n;
      for (int k = 0; k < 3; ++k) cX[c][k] = in ? obj[3 * i + k] : 0.0;
      for (int k = 0; k < 2; ++k) cU[c][k] = in ? img[2 * i + k] : 0.0;
      for (int k = 0; k < 3; ++k) cW[c][k] = in ? wgt[3 * i + k] : 0.0;  // a zero weight drops out of every sum
    }
  }
  int buf = 0;
  // one pass: the 30 sums at x, the same bits in every thread of the problem
  auto pass = [&](const double* x, double* S) {
    double R[9], Jl[9], v[WPNP_NS];
    wpnp_rot_and_jl(x, R, Jl);
    for (int k = 0; k < WPNP_NS; ++k) v[k] = 0.0;
    if (cached) {
      for (int c = 0; c < NC; ++c) wpnp_point(R, x + 3, Jl, fx, fy, cx, cy, cX[c], cU[c], cW[c], v);
    } else {
      for (int i = id; i < n; i += STRIDE) wpnp_point(R, x + 3, Jl, fx, fy, cx, cy, obj + 3 * i, img + 2 * i, wgt + 3 * i, v);
    }
    for (int k = 0; k < WPNP_NS; ++k) v[k] = wpnp_wave_allsum(v[k]);
    if (WAVE) {
      for (int k = 0; k < WPNP_NS; ++k) S[k] = v[k];
    } else {
      double* r = red + buf * (WPNP_WAVES * WPNP_NS);
      if (lane == 0)
        for (int k = 0; k < WPNP_NS; ++k) r[wave * WPNP_NS + k] = v[k];
      __syncthreads();
      for (int k = 0; k < WPNP_NS; ++k) {
        double s = r[k];
        for (int w = 1; w < WPNP_WAVES; ++w) s += r[w * WPNP_NS + k];
        S[k] = s;
      }
      buf ^= 1;
    }
  };

  double Ri[9], x[6], S[WPNP_NS];
  for (int k = 0; k < 9; ++k) Ri[k] = a.R_init[9 * prob + k];
  wpnp_log(Ri, x);
  for (int k = 0; k < 3; ++k) x[3 + k] = a.t_init[3 * prob + k];

  int status = -1, passes = 0;
  bool keep_start = false;
  double cost = 0.0, cost0 = 0.0;
  pass(x, S);
  if (S[29] < 3.0) {
    status = PP_WPNP_TOO_FEW;
    keep_start = true;
  } else {
    passes = 1;
    if (S[28] > 0.0) {
      status = PP_WPNP_BEHIND;
      keep_start = true;
    } else if (!wpnp_finite(S[27])) {
      status = PP_WPNP_SINGULAR;
      keep_start = true;
    }
  }
  if (status < 0) {
    cost = cost0 = S[27];
    double lam = 1e-4, nu = 2.0;
    double gmax = 0.0;
    for (int k = 0; k < 6; ++k) gmax = fmax(gmax, fabs(S[21 + k]));
    if (gmax < a.gtol) status = PP_WPNP_CONVERGED;
    while (status < 0) {
      if (passes - 1 >= a.max_iterations) {
        status = PP_WPNP_MAX_ITER;
        break;
      }
      double H[6][6], A[6][6], L[6][6], D[6], b[6], delta[6];
      int q = 0;
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c <= r; ++c, ++q) H[r][c] = H[c][r] = S[q];
      for (int r = 0; r < 6; ++r) {
        for (int c = 0; c < 6; ++c) A[r][c] = H[r][c];
        A[r][r] = H[r][r] + lam * fmin(fmax(H[r][r], 1e-6), 1e32);
        b[r] = -S[21 + r];
      }
      bool good = wpnp_ldlt(A, L, D);
      if (good) {
        wpnp_ldlt_solve(L, D, b, delta);
        for (int k = 0; k < 6; ++k) good = good && wpnp_finite(delta[k]);
      }
      if (!good) {
        status = PP_WPNP_SINGULAR;
        keep_start = true;
        break;
      }
      double d2 = 0.0, x2 = 0.0, gd = 0.0, dHd = 0.0;
      for (int k = 0; k < 6; ++k) {
        d2 += delta[k] * delta[k];
        x2 += x[k] * x[k];
        gd += S[21 + k] * delta[k];
        double hk = 0.0;
        for (int c = 0; c < 6; ++c) hk += H[k][c] * delta[c];
        dHd += delta[k] * hk;
      }
      if (sqrt(d2) <= a.ptol * (sqrt(x2) + a.ptol)) {
        status = PP_WPNP_CONVERGED;
        break;
      }
      const double pred = -gd - 0.5 * dHd;
      double xn[6], Sn[WPNP_NS];
      for (int k = 0; k < 6; ++k) xn[k] = x[k] + delta[k];
      pass(xn, Sn);
      ++passes;
      double rho = -1.0;
      if (!(Sn[28] > 0.0) && wpnp_finite(Sn[27]) && pred > 0.0) rho = (cost - Sn[27]) / pred;
      if (rho > 1e-3) {
        const double dcost = cost - Sn[27], cost_old = cost;
        for (int k = 0; k < 6; ++k) x[k] = xn[k];
        for (int k = 0; k < WPNP_NS; ++k) S[k] = Sn[k];
        cost = Sn[27];
        const double u = 2.0 * rho - 1.0;
        lam = fmin(fmax(lam * fmax(1.0 / 3.0, 1.0 - u * u * u), 1e-16), 1e32);
        nu = 2.0;
        gmax = 0.0;
        for (int k = 0; k < 6; ++k) gmax = fmax(gmax, fabs(S[21 + k]));
        if (gmax < a.gtol) {
          status = PP_WPNP_CONVERGED;
          break;
        }
        if (dcost <= a.ftol * cost_old) {
          status = PP_WPNP_CONVERGED;
          break;
        }
      } else {
        lam = fmin(lam * nu, 1e32);
        nu = 2.0 * nu;
      }
    }
  }
  if (id != 0) return;
  double Rf[9], Jl[9];
  if (keep_start) {
    for (int k = 0; k < 9; ++k) Rf[k] = Ri[k];
    for (int k = 0; k < 3; ++k) x[3 + k] = a.t_init[3 * prob + k];
    if (status != PP_WPNP_SINGULAR || passes < 1 || !wpnp_finite(cost0)) cost0 = 0.0;
    cost = cost0;
    wpnp_log(Ri, x);
  } else {
    wpnp_rot_and_jl(x, Rf, Jl);
  }
  for (int k = 0; k < 9; ++k) a.R_out[9 * prob + k] = Rf[k];
  for (int k = 0; k < 3; ++k) a.t_out[3 * prob + k] = x[3 + k];
  for (int k = 0; k < 3; ++k) a.rvec_out[3 * prob + k] = x[k];
  a.cost_init[prob] = cost0;
  a.cost_final[prob] = cost;
  a.iterations[prob] = passes;
  a.status[prob] = status;
  if (a.pose_cov) {
    double* C = a.pose_cov + 36 * (size_t)prob;
    double H[6][6], L[6][6], D[6];
    int q = 0;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c <= r; ++c, ++q) H[r][c] = H[c][r] = S[q];
    const bool good = !keep_start && wpnp_ldlt(H, L, D);
    for (int k = 0; k < 6; ++k) {
      double e[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, col[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      e[k] = 1.0;
      if (good) wpnp_ldlt_solve(L, D, e, col);
      for (int r = 0; r < 6; ++r) C[6 * r + k] = col[r];
    }
  }
}

// the problem's range, clamped to the arrays
__device__ __forceinline__ void wpnp_range(const WpnpArgs& a, int prob, int* p0, int* n) {
  int lo = a.offsets[prob], hi = a.offsets[prob + 1];
  lo = lo < 0 ? 0 : (lo > a.n_total ? a.n_total : lo);
  hi = hi < lo ? lo : (hi > a.n_total ? a.n_total : hi);
  *p0 = lo;
  *n = hi - lo;
}

__global__ __launch_bounds__(WPNP_THREADS) void wpnp_wave_kernel(const WpnpArgs a) {
  const int prob = blockIdx.x * WPNP_WAVES + (threadIdx.x >> 6);  // wave-uniform
  if (prob >= a.n_problems) return;
  int p0, n;
  wpnp_range(a, prob, &p0, &n);
  if (n > WPNP_WAVE_MAX) return;
  wpnp_problem<true>(a, prob, p0, n, nullptr);
}

__global__ __launch_bounds__(WPNP_THREADS) void wpnp_block_kernel(const WpnpArgs a) {
  __shared__ double red[2 * WPNP_WAVES * WPNP_NS];
  const int prob = blockIdx.x;
  int p0, n;
  wpnp_range(a, prob, &p0, &n);
  if (n <= WPNP_WAVE_MAX) return;  // block-uniform
  wpnp_problem<false>(a, prob, p0, n, red);
}

extern "C" size_t pp_pnp_refine_weighted_workspace_bytes(int n_problems, int n_points_total) {
  (void)n_problems;
  (void)n_points_total;
  return 0;
}

extern "C" int pp_pnp_refine_weighted_f64(pp_ctx* ctx, int n_problems, const int* offsets_dev, int n_points_total, const double* obj,
                                          const double* img, const double* wgt, const double* K4, const double* R_init,
                                          const double* t_init, int max_iterations, double gradient_tol, double parameter_tol,
                                          double function_tol, void* workspace, double* R_out, double* t_out, double* rvec_out,
                                          double* cost_init, double* cost_final, int* iterations, int* status, double* pose_cov) {
  PP_REQUIRE_CTX(ctx);
  (void)workspace;
  PP_CHECK_ARG(ctx, n_problems >= 0 && n_points_total >= 0 && max_iterations >= 0, PP_ERR_ARG, "pp_pnp_refine_weighted_f64: bad counts");
  PP_CHECK_ARG(ctx, n_problems <= (1 << 20), PP_ERR_ARG, "pp_pnp_refine_weighted_f64: at most 2^20 problems per call");
  PP_CHECK_ARG(ctx, gradient_tol >= 0.0 && parameter_tol >= 0.0 && function_tol >= 0.0, PP_ERR_ARG,
               "pp_pnp_refine_weighted_f64: tolerances must be >= 0");
  if (n_problems == 0) return PP_OK;
  PP_CHECK_ARG(ctx, offsets_dev && K4 && R_init && t_init && R_out && t_out && rvec_out && cost_init && cost_final && iterations && status &&
                        (n_points_total == 0 || (obj && img && wgt)),
               PP_ERR_ARG, "pp_pnp_refine_weighted_f64: null pointer");
  WpnpArgs a;
  a.n_problems = n_problems; a.n_total = n_points_total; a.offsets = offsets_dev; a.obj = obj; a.img = img; a.wgt = wgt; a.K4 = K4;
  a.R_init = R_init; a.t_init = t_init; a.max_iterations = max_iterations; a.gtol = gradient_tol; a.ptol = parameter_tol;
  a.ftol = function_tol; a.R_out = R_out; a.t_out = t_out; a.rvec_out = rvec_out; a.cost_init = cost_init; a.cost_final = cost_final;
  a.iterations = iterations; a.status = status; a.pose_cov = pose_cov;
  // both kernels see every problem and take the ones of their size class
  hipLaunchKernelGGL(wpnp_wave_kernel, dim3((unsigned)((n_problems + WPNP_WAVES - 1) / WPNP_WAVES)), dim3(WPNP_THREADS), 0, ctx->stream, a);
  PP_CHECK_LAUNCH(ctx, "pp_pnp_refine_weighted_f64 (wave path)");
  if (n_points_total > WPNP_WAVE_MAX) {
    hipLaunchKernelGGL(wpnp_block_kernel, dim3((unsigned)n_problems), dim3(WPNP_THREADS), 0, ctx->stream, a);
    PP_CHECK_LAUNCH(ctx, "pp_pnp_refine_weighted_f64 (workgroup path)");
  }
  return PP_OK;
}

// ---- vote statistics ----
struct VoteStatsArgs {
  int n_problems, n_total, ppv, mode;
  const int* offsets;
  const double* img;
  const double* vote_weight;        // [N / ppv] or NULL
  const unsigned char* mask;        // [N] or NULL
  double sigma2;
  double *wsum, *mu, *cov, *n_eff, *wgt;
  int* count;
};

__device__ void wpnp_weight_from_cov(double cxx, double cxy, double cyy, double n_eff, int mode, double sigma2, double* W) {
  W[0] = W[1] = W[2] = 0.0;
  if (mode == PP_WPNP_ISO) {
    if (cxx < 1e-5) return;
    const double m = 0.5 * (cxx + cyy), d = 0.5 * (cxx - cyy);
    const double w = 1.0 / (m + sqrt(d * d + cxy * cxy));
    W[0] = w;
    W[2] = w;
    return;
  }
  const double A = cxx / n_eff + sigma2, B = cxy / n_eff, C = cyy / n_eff + sigma2;
  const double m = 0.5 * (A + C), d = 0.5 * (A - C);
  const double r = sqrt(d * d + B * B);
  const double l1 = m + r, l2 = m - r;
  if (!(l2 > 0.0)) return;
  const double f1 = 1.0 / sqrt(l1), f2 = 1.0 / sqrt(l2);
  if (r == 0.0) {
    W[0] = f1;
    W[2] = f1;
    return;
  }
  const double k = (f1 - f2) / (2.0 * r);
  W[0] = f2 + k * (d + r);
  W[1] = k * B;
  W[2] = f2 + k * (r - d);
}

__global__ __launch_bounds__(WPNP_THREADS) void vote_stats_kernel(const VoteStatsArgs a) {
  const int prob = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int lo = a.offsets[prob], hi = a.offsets[prob + 1];
  lo = lo < 0 ? 0 : (lo > a.n_total ? a.n_total : lo);
  hi = hi < lo ? lo : (hi > a.n_total ? a.n_total : hi);
  const int ppv = a.ppv, k = (hi - lo) / ppv, v0 = lo / ppv;
  for (int j = wave; j < ppv; j += WPNP_WAVES) {  // wave-uniform
    double sw = 0.0, sw2 = 0.0, sx = 0.0, sy = 0.0, cnt = 0.0;
    for (int v = lane; v < k; v += 64) {
      const size_t i = (size_t)lo + (size_t)v * ppv + j;
      double w = a.vote_weight ? a.vote_weight[v0 + v] : 1.0;
      if (a.mask && !a.mask[i]) w = 0.0;
      if (!(w > 0.0)) continue;
      sw += w;
      sw2 += w * w;
      sx += w * a.img[2 * i];
      sy += w * a.img[2 * i + 1];
      cnt += 1.0;
    }
    sw = wpnp_wave_allsum(sw);
    sw2 = wpnp_wave_allsum(sw2);
    sx = wpnp_wave_allsum(sx);
    sy = wpnp_wave_allsum(sy);
    cnt = wpnp_wave_allsum(cnt);
    double mx = 0.0, my = 0.0, cxx = 0.0, cxy = 0.0, cyy = 0.0, ne = 0.0;
    if (cnt >= 1.0) {  // wave-uniform
      mx = sx / sw;
      my = sy / sw;
      for (int v = lane; v < k; v += 64) {
        const size_t i = (size_t)lo + (size_t)v * ppv + j;
        double w = a.vote_weight ? a.vote_weight[v0 + v] : 1.0;
        if (a.mask && !a.mask[i]) w = 0.0;
        if (!(w > 0.0)) continue;
        const double ex = a.img[2 * i] - mx, ey = a.img[2 * i + 1] - my;
        cxx += w * ex * ex;
        cxy += w * ex * ey;
        cyy += w * ey * ey;
      }
      cxx = wpnp_wave_allsum(cxx) / sw;
      cxy = wpnp_wave_allsum(cxy) / sw;
      cyy = wpnp_wave_allsum(cyy) / sw;
      ne = sw * sw / sw2;
    }
    if (lane == 0) {
      const size_t o = (size_t)prob * ppv + j;
      double W[3] = {0.0, 0.0, 0.0};
      if (cnt >= 2.0) wpnp_weight_from_cov(cxx, cxy, cyy, ne, a.mode, a.sigma2, W);
      a.wsum[o] = sw;
      a.count[o] = (int)cnt;
      a.mu[2 * o] = mx; a.mu[2 * o + 1] = my;
      a.cov[3 * o] = cxx; a.cov[3 * o + 1] = cxy; a.cov[3 * o + 2] = cyy;
      a.n_eff[o] = ne;
      a.wgt[3 * o] = W[0]; a.wgt[3 * o + 1] = W[1]; a.wgt[3 * o + 2] = W[2];
    }
  }
}

extern "C" size_t pp_vote_stats_workspace_bytes(int n_problems, int points_per_vote) {
  (void)n_problems;
  (void)points_per_vote;
  return 0;
}

extern "C" int pp_vote_stats_f64(pp_ctx* ctx, int n_problems, const int* offsets_dev, int n_points_total, const double* img,
                                 int points_per_vote, const double* vote_weight, const unsigned char* inlier_mask, int mode,
                                 double sigma_floor, void* workspace, double* wsum, int* count, double* mu, double* cov, double* n_eff,
                                 double* wgt) {
  PP_REQUIRE_CTX(ctx);
  (void)workspace;
  PP_CHECK_ARG(ctx, n_problems >= 0 && n_points_total >= 0 && n_problems <= (1 << 20), PP_ERR_ARG, "pp_vote_stats_f64: bad counts");
  PP_CHECK_ARG(ctx, points_per_vote >= 1 && points_per_vote <= 64 && n_points_total % points_per_vote == 0, PP_ERR_ARG,
               "pp_vote_stats_f64: points_per_vote must be 1..64 and divide the number of points");
  PP_CHECK_ARG(ctx, mode == PP_WPNP_FULL || mode == PP_WPNP_ISO, PP_ERR_ARG, "pp_vote_stats_f64: mode must be PP_WPNP_FULL or PP_WPNP_ISO");
  PP_CHECK_ARG(ctx, sigma_floor >= 0.0 && sigma_floor < 1e150, PP_ERR_ARG, "pp_vote_stats_f64: sigma_floor must be finite and >= 0");
  if (n_problems == 0) return PP_OK;
  PP_CHECK_ARG(ctx, offsets_dev && wsum && count && mu && cov && n_eff && wgt && (n_points_total == 0 || img), PP_ERR_ARG,
               "pp_vote_stats_f64: null pointer");
  VoteStatsArgs a;
  a.n_problems = n_problems; a.n_total = n_points_total; a.ppv = points_per_vote; a.mode = mode; a.offsets = offsets_dev; a.img = img;
  a.vote_weight = vote_weight; a.mask = inlier_mask; a.sigma2 = sigma_floor * sigma_floor;
  a.wsum = wsum; a.mu = mu; a.cov = cov; a.n_eff = n_eff; a.wgt = wgt; a.count = count;
  hipLaunchKernelGGL(vote_stats_kernel, dim3((unsigned)n_problems), dim3(WPNP_THREADS), 0, ctx->stream, a);
  PP_CHECK_LAUNCH(ctx, "pp_vote_stats_f64");
  return PP_OK;
}
