// The raster kernel of the colour renderer, included by render.hip once per kernel: the raster phase is
// render_raster_tile.inc (the depth pass's too); resolve, stores and shading are one text here and only the colour of the
// shading tail differs.  The includer defines RASTER_KERNEL (the kernel's name), RASTER_TEX (false: vertex colours
// [n_vert,3] in colors; true: texture coordinates [n_vert,2] there), RASTER_TP_PARAM (nothing, or the trailing tex_params
// parameter) and RASTER_TP (the tex_params the shading tail is given).  Two plain kernels rather than one template: the untextured
// one keeps the signature, the code and the place in the code object it had before the textured one existed.
__global__ void __launch_bounds__(RASTER_THREADS)
RASTER_KERNEL(int n_vert, const int* __restrict__ faces, const rvtx* __restrict__ vtx_all, int n_tri, int width, int height,
              int tiles_x, int n_tiles, const int* __restrict__ offsets, const int* __restrict__ list,
              const int* __restrict__ big_n, const int* __restrict__ big, double zn, double zf,
              const rattr* __restrict__ attr_all, const double* __restrict__ colors, rgb_params prm, float* __restrict__ depth,
              int* __restrict__ tri_id, float* __restrict__ rgb_f32, unsigned char* __restrict__ rgb_u8 RASTER_TP_PARAM) {
  __shared__ unsigned long long zb[RT * RT];
  __shared__ int queue[RASTER_THREADS];
  __shared__ int qn;
  const int pose = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const int r0 = (tile / tiles_x) * RT, c0 = (tile % tiles_x) * RT;
  const rvtx* vtx = vtx_all + (size_t)pose * n_vert;
#define RASTER_EMPTY ZKEY_EMPTY
#include "render_raster_tile.inc"
  // the tile, 4 pixels of one row per thread
  const int r = r0 + tid / (RT / 4), c = c0 + (tid % (RT / 4)) * 4;
  if (r >= height || c >= width) return;
  float z[4];
  int id[4];
  for (int k = 0; k < 4; ++k) {
    const unsigned long long key = zb[(tid / (RT / 4)) * RT + (tid % (RT / 4)) * 4 + k];
    const unsigned hi = (unsigned)(key >> 32);
    const bool hit = hi < 0x7F800000u;  // a depth that rounded to +inf is no fragment, as in the depth pass
    z[k] = hit ? __uint_as_float(hi) : 0.0f;
    id[k] = hit ? (int)(unsigned)key : -1;
  }
  const size_t px0 = ((size_t)pose * height + r) * width + c;
  const bool full = (width & 3) == 0;  // then c + 3 < width and px0 is a multiple of 4
  if (depth) {
    if (full && (reinterpret_cast<uintptr_t>(depth) & 15u) == 0) {
      *(float4*)(depth + px0) = make_float4(z[0], z[1], z[2], z[3]);
    } else {
      for (int k = 0; k < 4; ++k)
        if (c + k < width) depth[px0 + k] = z[k];
    }
  }
  if (tri_id) {
    if (full && (reinterpret_cast<uintptr_t>(tri_id) & 15u) == 0) {
      *(int4*)(tri_id + px0) = make_int4(id[0], id[1], id[2], id[3]);
    } else {
      for (int k = 0; k < 4; ++k)
        if (c + k < width) tri_id[px0 + k] = id[k];
    }
  }
  if (!rgb_f32 && !rgb_u8) return;
  float v[12];
  tri_shading<RASTER_TEX> S;
  int held = -1;
  for (int k = 0; k < 4; ++k) {
    if (id[k] < 0) {
      for (int j = 0; j < 3; ++j) v[3 * k + j] = (float)prm.bg[j];
      continue;
    }
    if (id[k] != held) {
      held = id[k];
      load_tri_shading<RASTER_TEX>(vtx, attr_all + (size_t)pose * n_vert, colors, n_vert, faces, held, width, height, prm.phong, &S);
    }
    shade_rgb_px<RASTER_TEX>(S, r, c + k, prm, RASTER_TP, v + 3 * k);
  }
  if (rgb_f32) {
    float* o = rgb_f32 + 3 * px0;
    if (full && (reinterpret_cast<uintptr_t>(rgb_f32) & 15u) == 0) {
      for (int j = 0; j < 3; ++j) ((float4*)o)[j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
    } else {
      for (int k = 0; k < 12; ++k)
        if (c + k / 3 < width) o[k] = v[k];
    }
  }
  if (rgb_u8) {
    unsigned char* o = rgb_u8 + 3 * px0;
    unsigned char u[12];
    for (int k = 0; k < 12; ++k) u[k] = rgb_to_u8(v[k]);
    if (full && (reinterpret_cast<uintptr_t>(rgb_u8) & 3u) == 0) {
      for (int j = 0; j < 3; ++j)
        ((unsigned*)o)[j] = (unsigned)u[4 * j] | ((unsigned)u[4 * j + 1] << 8) | ((unsigned)u[4 * j + 2] << 16) | ((unsigned)u[4 * j + 3] << 24);
    } else {
      for (int k = 0; k < 12; ++k)
        if (c + k / 3 < width) o[k] = u[k];
    }
  }
}
#undef RASTER_KERNEL
#undef RASTER_TEX
#undef RASTER_TP_PARAM
#undef RASTER_TP
