// Scene ground truth from rendered instances (masks, boxes, visibility) and a scene's image from its instances' colour renders.
//
// What bop_toolkit's calc_gt_masks / calc_gt_info write beforehand and annotation_scripts/annotate_BOP.py:363-378, 420, 461-471
// reads back (mask_visib/*.png, scene_gt_info.json), computed from the depth renders of a scene's instances.  Two passes:
//   1. scene:    per (scene, image pixel) the scene depth -- the given sensor depth or, without one, the nearest positive
//                instance depth -- then the id image: the scene's instances from the last to the first, the first one whose
//                'bop19' visibility mask holds the pixel wins, which is the later instance overwriting the earlier one
//                (annotate_BOP.py:373)
//   2. instance: per (instance, canvas pixel) the three pixel counts, both boxes and the optional masks; per-workgroup partials
//                (LDS integer atomics), then one wave per instance folds them
// A thread owns four pixels of a row whose image column is a multiple of 4: depths come in as one 16-byte load and bytes go out
// as one packed 4-byte store where the address allows, element by element otherwise.  Integer counts, minima and maxima only:
// the same bits whatever order the atomics run in.
// Compiled with -ffp-contract=off: the host restatement (tests/scene_gt_np.py) evaluates the same expressions in the same order.
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "pp_internal.h"
#include "visib_common.h"

#define SGT_THREADS 256
#define SGT_PART 11  // n_all, n_valid, n_visib, then (x_min, x_max, y_min, y_max) of the object and of its visible mask

// row[c0 .. c0 + 3] of a row of w floats, 0 where the column is outside [0, w)
__device__ __forceinline__ void load4_f32(const float* __restrict__ row, int c0, int w, float (&v)[4]) {
  if (c0 >= 0 && c0 + 3 < w && (reinterpret_cast<uintptr_t>(row + c0) & 15u) == 0) {
    const float4 q = *reinterpret_cast<const float4*>(row + c0);
    v[0] = q.x;
    v[1] = q.y;
    v[2] = q.z;
    v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (c0 + k >= 0 && c0 + k < w) ? row[c0 + k] : 0.0f;
  }
}

// the columns of v inside [0, w) to row[c0 .. c0 + 3]; c0 >= 0
__device__ __forceinline__ void store4_f32(float* __restrict__ row, int c0, int w, const float (&v)[4]) {
  if (c0 + 3 < w && (reinterpret_cast<uintptr_t>(row + c0) & 15u) == 0) {
    *reinterpret_cast<float4*>(row + c0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c0 + k < w) row[c0 + k] = v[k];
  }
}

__device__ __forceinline__ void store4_u8(unsigned char* __restrict__ row, int c0, int w, const unsigned char (&v)[4]) {
  if (c0 + 3 < w && (reinterpret_cast<uintptr_t>(row + c0) & 3u) == 0) {
    *reinterpret_cast<unsigned*>(row + c0) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c0 + k < w) row[c0 + k] = v[k];
  }
}

// the instances [i0, i1) of a scene; whatever the device copy of the offsets holds, the range stays inside the stack
__device__ __forceinline__ void scene_range(const int* __restrict__ scene_offsets, int scene, int n_inst, int* i0, int* i1) {
  *i0 = min(max(scene_offsets[scene], 0), n_inst);
  *i1 = min(max(scene_offsets[scene + 1], *i0), n_inst);
}

// grid (blocks of SGT_THREADS groups of 4 image pixels, scenes)
__global__ void __launch_bounds__(SGT_THREADS)
scene_gt_scene_kernel(int n_inst, int canvas_w, int canvas_h, int width, int height, int off_x, int off_y,
                      const float* __restrict__ stack, const int* __restrict__ scene_offsets, const float* __restrict__ depth_test,
                      long long test_stride, const double* __restrict__ K4, float delta, float* __restrict__ scene_depth,
                      unsigned char* __restrict__ id_image) {
  const int groups = (width + 3) / 4, gi = blockIdx.x * SGT_THREADS + threadIdx.x, scene = blockIdx.y;
  if (gi >= height * groups) return;
  const int r = gi / groups, c0 = (gi - r * groups) * 4;
  int i0, i1;
  scene_range(scene_offsets, scene, n_inst, &i0, &i1);
  const size_t cpx = (size_t)canvas_w * canvas_h, hw = (size_t)width * height;
  const float* win = stack + (size_t)(r + off_y) * canvas_w + off_x;  // row r of the window in instance 0's canvas
  float dt[4], dg[4];
  if (depth_test) {
    load4_f32(depth_test + (size_t)scene * test_stride + (size_t)r * width, c0, width, dt);
  } else {
    dt[0] = dt[1] = dt[2] = dt[3] = 0.0f;
    for (int i = i0; i < i1; ++i) {
      load4_f32(win + i * cpx, c0, width, dg);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (dg[k] > 0.0f && (dt[k] == 0.0f || dg[k] < dt[k])) dt[k] = dg[k];
    }
    store4_f32(scene_depth + scene * hw + (size_t)r * width, c0, width, dt);
  }
  unsigned char id[4] = {0, 0, 0, 0};
  int open = 0;  // bit k: pixel c0 + k is in the image and no instance has claimed it yet
#pragma unroll
  for (int k = 0; k < 4; ++k) open |= (c0 + k < width) ? 1 << k : 0;
  for (int i = i1 - 1; i >= i0 && open; --i) {
    load4_f32(win + i * cpx, c0, width, dg);
    const double* kk = K4 + 4 * (size_t)i;
    const double cx = kk[2], cy = kk[3], rfx = 1.0 / kk[0], rfy = 1.0 / kk[1];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!((open >> k) & 1) || !(dg[k] > 0.0f)) continue;
      const double t_ = dist_px(dt[k], r, c0 + k, cx, cy, rfx, rfy);
      const double g_ = dist_px(dg[k], r, c0 + k, cx, cy, rfx, rfy);
      if (visib_bop19(t_, g_, delta)) {
        id[k] = (unsigned char)(i - i0 + 1);
        open &= ~(1 << k);
      }
    }
  }
  store4_u8(id_image + scene * hw + (size_t)r * width, c0, width, id);
}

// grid (blocks of SGT_THREADS groups of 4 canvas pixels, instances).  A canvas row is cut into `groups` groups that start at
// canvas column 4 g - shift, shift = (4 - off_x % 4) % 4, so that a group's first image column is a multiple of 4.
// part [instance][block][SGT_PART]; box coordinates are image coordinates (canvas minus the window's offset).
__global__ void __launch_bounds__(SGT_THREADS)
scene_gt_inst_kernel(int n_scene, int canvas_w, int canvas_h, int width, int height, int off_x, int off_y, int shift, int groups,
                     const float* __restrict__ stack, const int* __restrict__ scene_offsets, const float* __restrict__ test,
                     long long test_stride, const double* __restrict__ K4, float delta, int* __restrict__ part,
                     unsigned char* __restrict__ mask_full, unsigned char* __restrict__ mask_visib) {
  __shared__ int acc[SGT_PART];
  const int tid = threadIdx.x, inst = blockIdx.y, gi = blockIdx.x * SGT_THREADS + tid;
  if (tid < SGT_PART) acc[tid] = tid < 3 ? 0 : (((tid - 3) & 1) ? INT_MIN : INT_MAX);
  __syncthreads();
  int n_all = 0, n_valid = 0, n_vis = 0;
  int ox0 = INT_MAX, ox1 = INT_MIN, oy0 = INT_MAX, oy1 = INT_MIN, vx0 = INT_MAX, vx1 = INT_MIN, vy0 = INT_MAX, vy1 = INT_MIN;
  if (gi < canvas_h * groups) {
    const int R = gi / groups, C0 = (gi - R * groups) * 4 - shift, r = R - off_y, c0 = C0 - off_x;  // c0 is a multiple of 4
    const bool row_in = r >= 0 && r < height;
    const size_t hw = (size_t)width * height;
    float dg[4], dt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    load4_f32(stack + (size_t)inst * canvas_w * canvas_h + (size_t)R * canvas_w, C0, canvas_w, dg);
    if (row_in) {
      int lo = 0, hi = n_scene;  // scene_offsets[lo] <= inst < scene_offsets[hi]; lo stays in [0, n_scene)
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (scene_offsets[mid] <= inst) lo = mid; else hi = mid;
      }
      load4_f32(test + (size_t)lo * test_stride + (size_t)r * width, c0, width, dt);
    }
    const double* kk = K4 + 4 * (size_t)inst;
    const double cx = kk[2], cy = kk[3], rfx = 1.0 / kk[0], rfy = 1.0 / kk[1];
    unsigned char mf[4], mv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + k;
      const bool gt = dg[k] > 0.0f;
      bool vis = false;
      if (gt) {
        ++n_all;
        ox0 = min(ox0, c);
        ox1 = max(ox1, c);
        oy0 = min(oy0, r);
        oy1 = max(oy1, r);
        if (row_in && c >= 0 && c < width) {
          n_valid += dt[k] > 0.0f ? 1 : 0;
          vis = visib_bop19(dist_px(dt[k], r, c, cx, cy, rfx, rfy), dist_px(dg[k], r, c, cx, cy, rfx, rfy), delta);
        }
      }
      if (vis) {
        ++n_vis;
        vx0 = min(vx0, c);
        vx1 = max(vx1, c);
        vy0 = min(vy0, r);
        vy1 = max(vy1, r);
      }
      mf[k] = gt ? 255 : 0;
      mv[k] = vis ? 255 : 0;
    }
    if (row_in && c0 >= 0 && c0 < width) {
      if (mask_full) store4_u8(mask_full + inst * hw + (size_t)r * width, c0, width, mf);
      if (mask_visib) store4_u8(mask_visib + inst * hw + (size_t)r * width, c0, width, mv);
    }
  }
  const int sums[3] = {wave_sum(n_all), wave_sum(n_valid), wave_sum(n_vis)};
  const int mins[4] = {wave_min(ox0), wave_min(oy0), wave_min(vx0), wave_min(vy0)};
  const int maxs[4] = {wave_max(ox1), wave_max(oy1), wave_max(vx1), wave_max(vy1)};
  if ((tid & 63) == 0) {
    for (int k = 0; k < 3; ++k) atomicAdd(&acc[k], sums[k]);
    // acc: obj x_min, x_max, y_min, y_max, visible x_min, x_max, y_min, y_max
    for (int k = 0; k < 4; ++k) {
      atomicMin(&acc[3 + 2 * k], mins[k]);
      atomicMax(&acc[4 + 2 * k], maxs[k]);
    }
  }
  __syncthreads();
  if (tid < SGT_PART) part[((size_t)inst * gridDim.x + blockIdx.x) * SGT_PART + tid] = acc[tid];
}

// one wave per instance: the blocks' partials -> px_count [3], bbox_obj (x, y, w, h), bbox_visib (x, y, w, h)
__global__ void __launch_bounds__(64)
scene_gt_final_kernel(int nblk, const int* __restrict__ part, long long* __restrict__ px_count, int* __restrict__ bbox_obj,
                      int* __restrict__ bbox_visib) {
  const int inst = blockIdx.x, lane = threadIdx.x;
  int v[SGT_PART];
#pragma unroll
  for (int k = 0; k < SGT_PART; ++k) v[k] = k < 3 ? 0 : (((k - 3) & 1) ? INT_MIN : INT_MAX);
  for (int b = lane; b < nblk; b += 64) {
    const int* p = part + ((size_t)inst * nblk + b) * SGT_PART;
#pragma unroll
    for (int k = 0; k < SGT_PART; ++k) v[k] = k < 3 ? v[k] + p[k] : (((k - 3) & 1) ? max(v[k], p[k]) : min(v[k], p[k]));
  }
#pragma unroll
  for (int k = 0; k < SGT_PART; ++k) v[k] = k < 3 ? wave_sum(v[k]) : (((k - 3) & 1) ? wave_max(v[k]) : wave_min(v[k]));
  if (lane != 0) return;
  for (int k = 0; k < 3; ++k) px_count[3 * (size_t)inst + k] = v[k];
  const bool seen = v[2] > 0;  // calc_gt_info: both boxes are (-1, -1, -1, -1) when nothing is visible
  for (int b = 0; b < 2; ++b) {
    int* box = (b ? bbox_visib : bbox_obj) + 4 * (size_t)inst;
    const int* m = v + 3 + 4 * b;  // x_min, x_max, y_min, y_max
    box[0] = seen ? m[0] : -1;
    box[1] = seen ? m[2] : -1;
    box[2] = seen ? m[1] - m[0] : -1;
    box[3] = seen ? m[3] - m[2] : -1;
  }
}

#define SGT_MAX_PER_SCENE 255  // the id image is uint8 and 0 is the background

static bool scene_gt_shape_ok(int n_inst, int canvas_w, int canvas_h) {
  return n_inst > 0 && n_inst <= 65535 && canvas_w > 0 && canvas_h > 0 && canvas_w <= 16384 && canvas_h <= 16384;
}

// the host copy of the offsets: from 0 to n_inst, never decreasing, no scene larger than the id image can name
static int scene_offsets_check(pp_ctx* ctx, const char* what, int n_inst, int n_scene, const int* scene_offsets_host) {
  PP_CHECK_ARG(ctx, scene_offsets_host[0] == 0 && scene_offsets_host[n_scene] == n_inst, PP_ERR_ARG,
               "%s: scene_offsets must run from 0 to n_inst", what);
  for (int s = 0; s < n_scene; ++s) {
    const int m = scene_offsets_host[s + 1] - scene_offsets_host[s];
    PP_CHECK_ARG(ctx, m >= 0, PP_ERR_ARG, "%s: scene_offsets must not decrease (scene %d)", what, s);
    PP_CHECK_ARG(ctx, m <= SGT_MAX_PER_SCENE, PP_ERR_SHAPE, "%s: scene %d has %d instances, the uint8 id image holds %d", what, s, m,
                 SGT_MAX_PER_SCENE);
  }
  return PP_OK;
}

// workgroups of scene_gt_inst_kernel per instance, at the window offset that needs the most groups per row
static size_t scene_gt_blocks(int canvas_w, int canvas_h, int shift) {
  const size_t groups = ((size_t)canvas_w + shift + 3) / 4;
  return (groups * canvas_h + SGT_THREADS - 1) / SGT_THREADS;
}

extern "C" size_t pp_scene_gt_workspace_bytes(int n_inst, int canvas_w, int canvas_h) {
  if (!scene_gt_shape_ok(n_inst, canvas_w, canvas_h)) return 0;
  return (size_t)n_inst * scene_gt_blocks(canvas_w, canvas_h, 3) * SGT_PART * sizeof(int);
}

extern "C" int pp_scene_gt_info(pp_ctx* ctx, int n_inst, int n_scene, const int* scene_offsets_host, const int* scene_offsets_dev,
                                int canvas_w, int canvas_h, int width, int height, int off_x, int off_y, const float* depth_stack,
                                const double* K4, const float* depth_test, long long test_stride, double delta, void* workspace,
                                size_t workspace_bytes, float* scene_depth, unsigned char* id_image, long long* px_count,
                                int* bbox_obj, int* bbox_visib, unsigned char* mask_full, unsigned char* mask_visib) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, scene_gt_shape_ok(n_inst, canvas_w, canvas_h) && n_scene > 0 && n_scene <= 65535, PP_ERR_SHAPE,
               "pp_scene_gt_info: need 1..65535 instances, 1..65535 scenes and a 1..16384 canvas");
  PP_CHECK_ARG(ctx, width > 0 && height > 0 && off_x >= 0 && off_y >= 0 && off_x <= canvas_w - width && off_y <= canvas_h - height,
               PP_ERR_SHAPE, "pp_scene_gt_info: the %d x %d window at (%d, %d) must lie inside the %d x %d canvas", width, height,
               off_x, off_y, canvas_w, canvas_h);
  PP_CHECK_ARG(ctx, scene_offsets_host && scene_offsets_dev && depth_stack && K4 && workspace && id_image && px_count && bbox_obj &&
                        bbox_visib, PP_ERR_ARG, "pp_scene_gt_info: null argument");
  PP_CHECK_ARG(ctx, (depth_test != nullptr) != (scene_depth != nullptr), PP_ERR_ARG,
               "pp_scene_gt_info: give depth_test, or scene_depth for the depth composed from the instances, not both");
  PP_CHECK_ARG(ctx, !depth_test || test_stride == 0 || test_stride == (long long)width * height, PP_ERR_ARG,
               "pp_scene_gt_info: test_stride must be 0 (one depth image shared by the scenes) or width * height");
  PP_CHECK_ARG(ctx, delta >= 0.0, PP_ERR_ARG, "pp_scene_gt_info: delta must not be negative");  // (a NaN is refused too)
  const int rc = scene_offsets_check(ctx, "pp_scene_gt_info", n_inst, n_scene, scene_offsets_host);
  if (rc) return rc;
  const int shift = (4 - off_x % 4) % 4, groups = (canvas_w + shift + 3) / 4;
  const size_t nblk = scene_gt_blocks(canvas_w, canvas_h, shift), need = (size_t)n_inst * nblk * SGT_PART * sizeof(int);
  PP_CHECK_ARG(ctx, workspace_bytes >= need, PP_ERR_ARG, "pp_scene_gt_info: workspace of %zu bytes, need %zu", workspace_bytes, need);
  const size_t hw = (size_t)width * height;
  const int scene_blocks = (int)((((size_t)width + 3) / 4 * height + SGT_THREADS - 1) / SGT_THREADS);
  hipLaunchKernelGGL(scene_gt_scene_kernel, dim3(scene_blocks, n_scene), dim3(SGT_THREADS), 0, ctx->stream, n_inst, canvas_w, canvas_h,
                     width, height, off_x, off_y, depth_stack, scene_offsets_dev, depth_test, test_stride, K4, (float)delta, scene_depth,
                     id_image);
  const float* test = depth_test ? depth_test : scene_depth;
  hipLaunchKernelGGL(scene_gt_inst_kernel, dim3((unsigned)nblk, n_inst), dim3(SGT_THREADS), 0, ctx->stream, n_scene, canvas_w, canvas_h,
                     width, height, off_x, off_y, shift, groups, depth_stack, scene_offsets_dev, test,
                     depth_test ? test_stride : (long long)hw, K4, (float)delta, (int*)workspace, mask_full, mask_visib);
  hipLaunchKernelGGL(scene_gt_final_kernel, dim3(n_inst), dim3(64), 0, ctx->stream, (int)nblk, (const int*)workspace, px_count, bbox_obj,
                     bbox_visib);
  PP_CHECK_LAUNCH(ctx, "pp_scene_gt_info");
  return PP_OK;
}

// ---- a scene's image from its instances' colour renders ---------------------------------------------------------------------
// Per (scene, pixel): id k > 0 of pp_scene_gt_info's id image selects the colour of instance scene_offsets[scene] + k - 1 of
// the uint8 stack (pp_render_rgbd outputs in scene order), anything else the background -- the scene's image or a constant.
// Inputs are RGB; the output is RGB or, reversed per pixel, BGR.  A thread owns four pixels of a row (one packed load of the
// ids, three packed stores where the addresses allow).  Bytes are selected, never computed.
__global__ void __launch_bounds__(SGT_THREADS)
scene_compose_kernel(int n_inst, int width, int height, const int* __restrict__ scene_offsets, const unsigned char* __restrict__ id_image,
                     const unsigned char* __restrict__ colors, const unsigned char* __restrict__ background, unsigned bg_const, int bgr,
                     unsigned char* __restrict__ out) {
  const int groups = (width + 3) / 4, gi = blockIdx.x * SGT_THREADS + threadIdx.x, scene = blockIdx.y;
  if (gi >= height * groups) return;
  const int r = gi / groups, c0 = (gi - r * groups) * 4;
  int i0, i1;
  scene_range(scene_offsets, scene, n_inst, &i0, &i1);
  const size_t hw = (size_t)width * height, p0 = (size_t)r * width + c0;
  const unsigned char* ids = id_image + scene * hw + p0;
  const bool whole = c0 + 3 < width;
  unsigned packed = 0;
  if (whole && (reinterpret_cast<uintptr_t>(ids) & 3u) == 0) {
    packed = *reinterpret_cast<const unsigned*>(ids);
  } else {
    for (int k = 0; k < 4; ++k)
      if (c0 + k < width) packed |= (unsigned)ids[k] << (8 * k);
  }
  unsigned char v[12];
  for (int k = 0; k < 4; ++k) {
    const int id = (int)((packed >> (8 * k)) & 255u);
    const unsigned char* src = nullptr;
    if (c0 + k < width) {
      if (id > 0 && id <= i1 - i0)
        src = colors + ((size_t)(i0 + id - 1) * hw + p0 + k) * 3;
      else if (background)
        src = background + (scene * hw + p0 + k) * 3;
    }
    for (int j = 0; j < 3; ++j) {
      const int jj = bgr ? 2 - j : j;
      v[3 * k + j] = src ? src[jj] : (unsigned char)((bg_const >> (8 * jj)) & 255u);
    }
  }
  unsigned char* o = out + (scene * hw + p0) * 3;
  if (whole && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
    for (int j = 0; j < 3; ++j)
      reinterpret_cast<unsigned*>(o)[j] = (unsigned)v[4 * j] | ((unsigned)v[4 * j + 1] << 8) | ((unsigned)v[4 * j + 2] << 16) | ((unsigned)v[4 * j + 3] << 24);
  } else {
    for (int k = 0; k < 12; ++k)
      if (c0 + k / 3 < width) o[k] = v[k];
  }
}

extern "C" int pp_scene_compose_u8(pp_ctx* ctx, int n_inst, int n_scene, const int* scene_offsets_host, const int* scene_offsets_dev,
                                   int width, int height, const unsigned char* id_image, const unsigned char* colors,
                                   const unsigned char* background, const unsigned char* bg_const, int channel_order,
                                   unsigned char* out) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, scene_gt_shape_ok(n_inst, width, height) && n_scene > 0 && n_scene <= 65535, PP_ERR_SHAPE,
               "pp_scene_compose_u8: need 1..65535 instances, 1..65535 scenes and a 1..16384 image");
  PP_CHECK_ARG(ctx, scene_offsets_host && scene_offsets_dev && id_image && colors && out && (background || bg_const), PP_ERR_ARG,
               "pp_scene_compose_u8: null argument (give a background image or a constant)");
  PP_CHECK_ARG(ctx, channel_order == 0 || channel_order == 1, PP_ERR_ARG, "pp_scene_compose_u8: channel_order must be 0 (RGB) or 1 (BGR)");
  const int rc = scene_offsets_check(ctx, "pp_scene_compose_u8", n_inst, n_scene, scene_offsets_host);
  if (rc) return rc;
  const unsigned bg = background ? 0u : (unsigned)bg_const[0] | ((unsigned)bg_const[1] << 8) | ((unsigned)bg_const[2] << 16);
  const int blocks = (int)((((size_t)width + 3) / 4 * height + SGT_THREADS - 1) / SGT_THREADS);
  hipLaunchKernelGGL(scene_compose_kernel, dim3(blocks, n_scene), dim3(SGT_THREADS), 0, ctx->stream, n_inst, width, height,
                     scene_offsets_dev, id_image, colors, background, bg, channel_order, out);
  PP_CHECK_LAUNCH(ctx, "pp_scene_compose_u8");
  return PP_OK;
}
