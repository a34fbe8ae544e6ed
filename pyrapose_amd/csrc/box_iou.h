// The two 2-D box overlaps of the library, shared by anchors.hip (pp_compute_overlap_f64, the target assignment) and
// det_eval.hip (pp_det_match).  Boxes are (x1, y1, x2, y2) in float64; every includer is compiled with -ffp-contract=off, so
// each product and sum is rounded on its own.
#pragma once
#include "pp_internal.h"

// utils/compute_overlap.pyx:13-53 with its "+1" pixel convention: b is a row of `boxes`, q a row of `query_boxes`,
// q_area = (qx2 - qx1 + 1) * (qy2 - qy1 + 1)
__device__ __forceinline__ double iou_plus1(double bx1, double by1, double bx2, double by2, double qx1, double qy1, double qx2,
                                            double qy2, double q_area) {
  const double iw = fmin(bx2, qx2) - fmax(bx1, qx1) + 1;
  if (!(iw > 0)) return 0.0;
  const double ih = fmin(by2, qy2) - fmax(by1, qy1) + 1;
  if (!(ih > 0)) return 0.0;
  const double ua = (bx2 - bx1 + 1) * (by2 - by1 + 1) + q_area - iw * ih;
  return iw * ih / ua;
}

// pycocotools' bbIou without crowd, restated on corner boxes (w = x2 - x1, h = y2 - y1, no "+1"): d is the detection, g the
// ground truth, g_area = (gx2 - gx1) * (gy2 - gy1); u = d_area + g_area - i in that association
__device__ __forceinline__ double iou_plain(double dx1, double dy1, double dx2, double dy2, double gx1, double gy1, double gx2,
                                            double gy2, double g_area) {
  const double iw = fmin(dx2, gx2) - fmax(dx1, gx1);
  if (!(iw > 0)) return 0.0;
  const double ih = fmin(dy2, gy2) - fmax(dy1, gy1);
  if (!(ih > 0)) return 0.0;
  const double i = iw * ih;
  const double u = (dx2 - dx1) * (dy2 - dy1) + g_area - i;
  return i / u;
}
