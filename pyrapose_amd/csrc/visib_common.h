// What VSD (vsd.hip) and scene ground truth (scene_gt.hip) share: a depth pixel's distance from the camera, the two visibility
// rules and the 64-lane integer butterflies.  Both includers are compiled with -ffp-contract=off.
#pragma once
#include <math.h>

// depth_im_to_dist_im (pose_error.py:43-61) at one pixel: || ((c - cx) d / fx, (r - cy) d / fy, d) ||, summed x, y, z in order
__device__ __forceinline__ double dist_px(float d, int r, int c, double cx, double cy, double rfx, double rfy) {
  const double dd = (double)d;
  const double X = (((double)c - cx) * dd) * rfx;
  const double Y = (((double)r - cy) * dd) * rfy;
  return sqrt((X * X + Y * Y) + dd * dd);
}

// estimate_visib_mask (pose_error.py:15-29): both valid and float32(d_model) - float32(d_test) <= delta (in float32)
__device__ __forceinline__ bool visib(double d_test, double d_model, float delta) {
  return d_test > 0.0 && d_model > 0.0 && ((float)d_model - (float)d_test) <= delta;
}

// BOP 2019 (bop_toolkit's estimate_visib_mask with visib_mode 'bop19'; parity with bop_toolkit unpinned): a rendered pixel
// without a sensor value counts as visible
__device__ __forceinline__ bool visib_bop19(double d_test, double d_model, float delta) {
  return d_model > 0.0 && (((float)d_model - (float)d_test) <= delta || d_test == 0.0);
}

__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ int wave_min(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ int wave_max(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
