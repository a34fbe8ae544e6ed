// The weight-gradient kernels of the plane-format convolution family -- wgrad3, wgrad3f and the slice finish -- and their launcher
// (conv3.h).  The tap-row-reuse forms wgrad3r / wgrad3w are in conv4.hip; the arithmetic is described at the head of conv3.hip.
#include "conv3_unit.h"
#include "conv3.h"

namespace {

typedef short shortx4 __attribute__((ext_vector_type(4)));

// ---- wgrad3: weight gradient on the bf16 matrix cores:  dw[tap][ci][co] += sum_m x[gather(m,tap)][ci] * dy[m][co]
// The reduction index is the pixel m, but NHWC tensors are channel-contiguous, so both MFMA operands need a
// transpose: the 32-pixel x 128-channel f32 tiles are split to bf16 (hi, lo) while they are staged into LDS
// pixel-major ([pixel][channel], pitch = row + 64 B) and the k-contiguous fragments are fetched with the
// transposing LDS read ds_read_b64_tr_b16 (two reads = 8 pixels of one channel per lane; lane map verified by
// tools/ubench/tr16_check.hip).  With the +64 B pitch the four rows of a 16-lane read group fall in four disjoint
// 16-dword bank windows: conflict free.  Split over pixel ranges + f32 atomics like wgrad_kernel (conv.hip).
template <int TM, int TN, bool AP>
__global__ __launch_bounds__(256, (TM * TN == 4) ? 2 : 3) void wgrad3_kernel(const Wgrad3Params p, const float* __restrict__ g_src,
                                                                            const float* __restrict__ g_dy,
                                                                            const uint4* __restrict__ g_xhi, const uint4* __restrict__ g_xlo,
                                                                            const uint4* __restrict__ g_dhi, const uint4* __restrict__ g_dlo,
                                                                            float* __restrict__ g_dw, float* __restrict__ g_dbias) {
  constexpr int BM = 64 * TM, BN = 64 * TN, BK = 32;
  constexpr int PA = BM + 32, PB = BN + 32;  // LDS pitches in bf16 elements (row + 64 bytes)
  __shared__ __attribute__((aligned(16))) unsigned short smem[2 * BK * (PA + PB)];
  unsigned short* Xhi = smem;
  unsigned short* Xlo = Xhi + BK * PA;
  unsigned short* Ghi = Xlo + BK * PA;
  unsigned short* Glo = Ghi + BK * PB;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float inv_g = p.inv_scale ? *p.inv_scale : 1.f;
  const int wm = wave >> 1, wn = wave & 1;
  int b = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int tile_n = b % p.n_tiles_n;
  b /= p.n_tiles_n;
  const int tile_k = b % p.n_tiles_k;
  const int split = b / p.n_tiles_k;
  const int tap = tile_k / p.k_tiles_per_tap;
  const int ci0 = (tile_k - tap * p.k_tiles_per_tap) * BM;
  const int ty = tap / p.kw, tx = tap - ty * p.kw;
  const int n0 = tile_n * BN;
  const int m_begin = split * p.rows_per_split;
  const int m_end = min(p.M, m_begin + p.rows_per_split);
  const int n_steps = (m_end - m_begin + BK - 1) / BK;

  // staging: 8 threads per pixel row, thread loads the float4 channel quads q8 + 8*j
  const int prow = tid >> 3, q8 = tid & 7;
  constexpr int QA = BM / 32, QB = BN / 32;  // quads per thread
  struct WRow { int m, n, y, x, seg_end, sb, OH, OW, SH, SW; } w;
  auto decode = [&](int m) {
    w.m = m;
    int rbeg = p.seg[0].row_begin;
    w.sb = p.seg[0].src_row_begin; w.OH = p.seg[0].OH; w.OW = p.seg[0].OW; w.SH = p.seg[0].SH; w.SW = p.seg[0].SW;
    w.seg_end = p.n_seg > 1 ? p.seg[1].row_begin : p.M;
    for (int s = 1; s < p.n_seg; ++s) {
      if (m >= p.seg[s].row_begin) {
        rbeg = p.seg[s].row_begin; w.sb = p.seg[s].src_row_begin; w.OH = p.seg[s].OH; w.OW = p.seg[s].OW;
        w.SH = p.seg[s].SH; w.SW = p.seg[s].SW;
        w.seg_end = (s + 1 < p.n_seg) ? p.seg[s + 1].row_begin : p.M;
      }
    }
    const int local = m < p.M ? m - rbeg : 0;
    const int hw = w.OH * w.OW;
    w.n = local / hw;
    const int rem = local - w.n * hw;
    w.y = rem / w.OW;
    w.x = rem - w.y * w.OW;
  };
  decode(m_begin + prow);

  constexpr int OA = (BM / 64 > 0) ? BM / 64 : 1, OB = (BN / 64 > 0) ? BN / 64 : 1;  // 8-channel chunks per thread (AP)
  float4 ra[QA], rb[QB];
  uint4 pah[OA], pal[OA], pbh[OB], pbl[OB];
  float4 bsum[QB];
#pragma unroll
  for (int j = 0; j < QB; ++j) bsum[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool do_bias = (g_dbias != nullptr) && (tile_k == 0);

  auto load_step = [&]() {
    const int sy = w.y * p.stride + ty - p.pad_t;
    const int sx = w.x * p.stride + tx - p.pad_l;
    const bool in_rng = w.m < m_end;
    const bool ok = in_rng && ((unsigned)sy < (unsigned)w.SH) && ((unsigned)sx < (unsigned)w.SW);
    const long long xrow = (long long)(w.sb + w.n * w.SH * w.SW + sy * w.SW + sx) * p.ld_src + ci0;
    if (AP) {
#pragma unroll
      for (int j = 0; j < OA; ++j) {
        const long long o8 = 2 * ((xrow >> 3) + q8 + 8 * j);  // packed planes: 32-byte groups
        pah[j] = ok ? g_xhi[o8] : make_uint4(0u, 0u, 0u, 0u);
        pal[j] = ok ? g_xlo[o8] : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int j = 0; j < OB; ++j) {
        const int c = n0 + 8 * (q8 + 8 * j);
        const bool okb = in_rng && c < p.ld_dy;
        const long long o8 = 2 * ((((long long)w.m * p.ld_dy + n0) >> 3) + q8 + 8 * j);
        pbh[j] = okb ? g_dhi[o8] : make_uint4(0u, 0u, 0u, 0u);
        pbl[j] = okb ? g_dlo[o8] : make_uint4(0u, 0u, 0u, 0u);
      }
    } else {
      const float* src = g_src + xrow;
#pragma unroll
      for (int j = 0; j < QA; ++j)
        ra[j] = ok ? *reinterpret_cast<const float4*>(src + 4 * (q8 + 8 * j)) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float* dyr = g_dy + (long long)w.m * p.ld_dy + n0;
#pragma unroll
      for (int j = 0; j < QB; ++j) {
        const int c = n0 + 4 * (q8 + 8 * j);
        rb[j] = (in_rng && c < p.ld_dy) ? *reinterpret_cast<const float4*>(dyr + 4 * (q8 + 8 * j)) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    // advance this thread's pixel row by one step
    const int m2 = w.m + BK;
    if (m2 >= w.seg_end) {
      decode(m2);
    } else {
      w.m = m2;
      w.x += BK;
      while (w.x >= w.OW) { w.x -= w.OW; ++w.y; }
      while (w.y >= w.OH) { w.y -= w.OH; ++w.n; }
    }
  };
  auto store_step = [&]() {
    if (AP) {
#pragma unroll
      for (int j = 0; j < OA; ++j) {
        const int off = prow * PA + 8 * (q8 + 8 * j);
        if (8 * (q8 + 8 * j) < BM) {
          *reinterpret_cast<uint4*>(Xhi + off) = pah[j];
          *reinterpret_cast<uint4*>(Xlo + off) = pal[j];
        }
      }
#pragma unroll
      for (int j = 0; j < OB; ++j) {
        const int off = prow * PB + 8 * (q8 + 8 * j);
        if (8 * (q8 + 8 * j) < BN) {
          *reinterpret_cast<uint4*>(Ghi + off) = pbh[j];
          *reinterpret_cast<uint4*>(Glo + off) = pbl[j];
          if (do_bias) {  // dy = hi + lo (2^-17): only the workgroups of the first k-tile pay for this
            const unsigned int hw[4] = {pbh[j].x, pbh[j].y, pbh[j].z, pbh[j].w}, lw[4] = {pbl[j].x, pbl[j].y, pbl[j].z, pbl[j].w};
            float v[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) fmt_value2(hw[e], lw[e], &v[2 * e], &v[2 * e + 1]);
            bsum[2 * j].x += v[0]; bsum[2 * j].y += v[1]; bsum[2 * j].z += v[2]; bsum[2 * j].w += v[3];
            bsum[2 * j + 1].x += v[4]; bsum[2 * j + 1].y += v[5]; bsum[2 * j + 1].z += v[6]; bsum[2 * j + 1].w += v[7];
          }
        }
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < QA; ++j) {
      uint2 hi, lo;
      split4(ra[j], &hi, &lo);
      const int off = prow * PA + 4 * (q8 + 8 * j);
      *reinterpret_cast<uint2*>(Xhi + off) = hi;
      *reinterpret_cast<uint2*>(Xlo + off) = lo;
    }
#pragma unroll
    for (int j = 0; j < QB; ++j) {
      uint2 hi, lo;
      split4(rb[j], &hi, &lo);
      const int off = prow * PB + 4 * (q8 + 8 * j);
      *reinterpret_cast<uint2*>(Ghi + off) = hi;
      *reinterpret_cast<uint2*>(Glo + off) = lo;
      if (do_bias) { bsum[j].x += rb[j].x; bsum[j].y += rb[j].y; bsum[j].z += rb[j].z; bsum[j].w += rb[j].w; }
    }
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int c = 0; c < TN; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;

  // transposed-read lane roles (16-lane groups): group g -> columns 16*(g&1).., pixel half h = g>>1
  const int grp = lane >> 4, gi = lane & 15, gq = gi >> 2, gp = gi & 3;
  const int cbase = 16 * (grp & 1), hh = grp >> 1;
  const int il = lane & 31, h = lane >> 5;

  if (n_steps > 0) {
    load_step();
    store_step();
  }
  __syncthreads();
  for (int step = 0; step < n_steps; ++step) {
    const bool more = step + 1 < n_steps;
    if (more) load_step();
    wgrad_step<TM, TN>(acc, Xhi, Xlo, Ghi, Glo, PA, PB, wm * 32 * TM + cbase + 4 * gp, wn * 32 * TN + cbase + 4 * gp, hh, gq);
    __syncthreads();
    if (more) {
      store_step();
      __syncthreads();
    }
  }

#pragma unroll
  for (int a = 0; a < TM; ++a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = ci0 + wm * 32 * TM + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      float* dst = g_dw + (long long)(tap * p.Cin + ci) * p.ld_w;
#pragma unroll
      for (int c = 0; c < TN; ++c) {
        const int co = n0 + wn * 32 * TN + c * 32 + il;
        if (co < p.Cout) atomicAdd(dst + co, acc[a][c][r] * inv_g);
      }
    }
  }
  if (do_bias) {
    // 32 threads (one per pixel row of the step) hold partial sums of the same channel quad: reduce through LDS
    float* red = reinterpret_cast<float*>(smem);  // [32][BN] floats <= LDS size
    __syncthreads();
    if (AP) {
#pragma unroll
      for (int j = 0; j < OB; ++j)
        if (8 * (q8 + 8 * j) < BN) {
          *reinterpret_cast<float4*>(red + prow * BN + 8 * (q8 + 8 * j)) = bsum[2 * j];
          *reinterpret_cast<float4*>(red + prow * BN + 8 * (q8 + 8 * j) + 4) = bsum[2 * j + 1];
        }
    } else {
#pragma unroll
      for (int j = 0; j < QB; ++j) *reinterpret_cast<float4*>(red + prow * BN + 4 * (q8 + 8 * j)) = bsum[j];
    }
    __syncthreads();
    if (tid < BN) {
      float s = 0.f;
#pragma unroll 8
      for (int r = 0; r < 32; ++r) s += red[r * BN + tid];
      if (n0 + tid < p.Cout) atomicAdd(g_dbias + n0 + tid, s * inv_g);
    }
  }
}

// ---- wgrad3f: the same tiles with a branch-free k-loop (see igemm3f_kernel) ----
// Every step each staging thread re-derives (image, y, x) of its pixel row from m with two reciprocal divisions
// (exact for m < 2^24, host-checked) instead of the incremental walk with its data-dependent loops, addresses both
// operands with 32-bit buffer offsets (out-of-range = zeros: padding taps, rows past the split, columns past ld_dy)
// and converts the loaded tile while its MFMAs drain.  No 64-bit address registers -> 3 workgroups per CU at 128x128.

// SP: the reduction walks a LIST of 32-row blocks (pp_row_block_list: the blocks of dy that hold a non-zero) instead of all
// rows -- the gradient of the 3D-box head is non-zero only around positive anchors (losses.py:332-333 keeps state == 1
// rows), and a block of zero rows adds exactly nothing to dW.  list[0] = number of blocks, list[1..] ascending; the
// splits share the list evenly, so the launch stays balanced whatever the data.
template <int TM, int TN, bool AP, bool SP>
__global__ __launch_bounds__(256, (TM * TN == 4) ? 3 : 4) void wgrad3f_kernel(const Wgrad3Params p, const void* __restrict__ g_x0,
                                                                            const void* __restrict__ g_x1, unsigned x_bytes,
                                                                            const void* __restrict__ g_d0, const void* __restrict__ g_d1,
                                                                            unsigned d_bytes, float* __restrict__ g_dw,
                                                                            float* __restrict__ g_dbias, const int* __restrict__ g_list,
                                                                            float* __restrict__ g_ws, long long ws_slice) {
  constexpr int BM = 64 * TM, BN = 64 * TN, BK = 32;
  constexpr int PA = BM + 32, PB = BN + 32;  // LDS pitches in bf16 elements (row + 64 bytes)
  constexpr int ES = 4;              // f32, or packed planes (32-byte groups of 8 channels: hi, then lo = the *1 resources)
  constexpr int CB = AP ? 32 : 16;   // bytes between the 16-byte chunks a staging thread fetches from one resource
  __shared__ __attribute__((aligned(16))) unsigned short smem[2 * BK * (PA + PB)];
  unsigned short* Xhi = smem;
  unsigned short* Xlo = Xhi + BK * PA;
  unsigned short* Ghi = Xlo + BK * PA;
  unsigned short* Glo = Ghi + BK * PB;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float inv_g = p.inv_scale ? *p.inv_scale : 1.f;
  const int wm = wave >> 1, wn = wave & 1;
  int b = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int tile_n = b % p.n_tiles_n;
  b /= p.n_tiles_n;
  const int tile_k = b % p.n_tiles_k;
  const int split = b / p.n_tiles_k;
  const int tap = tile_k / p.k_tiles_per_tap;
  const int ci0 = (tile_k - tap * p.k_tiles_per_tap) * BM;
  const int ty = tap / p.kw, tx = tap - ty * p.kw;
  const int n0 = tile_n * BN;
  int m_begin = split * p.rows_per_split;
  int m_end = min(p.M, m_begin + p.rows_per_split);
  int n_steps = (m_end - m_begin + BK - 1) / BK;
  int s_idx = 0, s_end = 0;
  const int blk_past = (p.M + BK - 1) / BK;  // SP: "no more blocks" (its rows are >= M: loads return zeros)
  if (SP) {
    // The grid was sized on the host for the dense reduction; a short list is shared by FEWER splits (uniform early exit of
    // the others, before any barrier): every split adds a full |dW| tile set with float atomics, which at 12 blocks per
    // split cost more than the reduction itself (3D-box head on the bench targets: 16 splits x 9.4 MB of atomics for ~200
    // listed blocks).  The slices of the deterministic mode need every split's slice written: no reduction there.
    const int n_act = g_list[0];
    int s_eff = (n_act + p.sp_min_steps - 1) / p.sp_min_steps;
    s_eff = s_eff < 1 ? 1 : (s_eff > p.splits ? p.splits : s_eff);
    if (g_ws) s_eff = p.splits;
    if (split >= s_eff) return;
    s_idx = (int)((long long)n_act * split / s_eff);
    s_end = (int)((long long)n_act * (split + 1) / s_eff);
    n_steps = s_end - s_idx;
    m_begin = (n_steps > 0 ? g_list[1 + s_idx] : blk_past) * BK;
    m_end = p.M;
  }

  const __amdgpu_buffer_rsrc_t rs_x0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g_x0), 0, x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_x1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(AP ? g_x1 : g_x0), 0, AP ? x_bytes - 16 : x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_d0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g_d0), 0, d_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_d1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(AP ? g_d1 : g_d0), 0, AP ? d_bytes - 16 : d_bytes, 0x00020000);

  // staging: 8 threads per pixel row; thread q8 loads the 16-byte chunks q8 + 8*j of its row
  const int prow = tid >> 3, q8 = tid & 7;
  constexpr int QA = AP ? (BM / 64) : (BM / 32), QB = AP ? (BN / 64) : (BN / 32);  // 16-byte chunks per thread and operand
  constexpr int CH = AP ? 8 : 4;                                                    // channels per chunk
  uint4 ra[QA], rb[QB];                // f32 quads, or bf16 hi chunks (AP)
  uint4 ral[AP ? QA : 1], rbl[AP ? QB : 1];  // bf16 lo chunks (AP)
  uint2 sah[AP ? 1 : QA], sal[AP ? 1 : QA], sbh[AP ? 1 : QB], sbl[AP ? 1 : QB];  // converted tile (f32 path)
  float4 bsum[BN / 32];
#pragma unroll
  for (int j = 0; j < BN / 32; ++j) bsum[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool do_bias = (g_dbias != nullptr) && (tile_k == 0);
  // Per-thread walk over its pixel rows m = m_begin + prow + 32 * step: (image base, y, x) advance incrementally
  // (x += 32 with a bounded number of row wraps; wraps = ceil(32 / narrowest level)); only when a lane crosses into
  // the next pyramid level does the wave take the (wave-uniform, rare) full decode.
  int m_cur = m_begin + prow;
  int c_OW, c_OH, c_SW, c_SH, c_end, r_x, r_y, r_img;  // level constants and position of row m_cur
  auto decode = [&](int m) {
    int rbeg = p.seg[0].row_begin, sb = p.seg[0].src_row_begin;
    c_OH = p.seg[0].OH; c_OW = p.seg[0].OW; c_SH = p.seg[0].SH; c_SW = p.seg[0].SW;
    c_end = p.n_seg > 1 ? p.seg[1].row_begin : 0x7fffffff;
    for (int s = 1; s < p.n_seg; ++s) {
      const bool in = m >= p.seg[s].row_begin;
      rbeg = in ? p.seg[s].row_begin : rbeg;
      sb = in ? p.seg[s].src_row_begin : sb;
      c_OH = in ? p.seg[s].OH : c_OH;
      c_OW = in ? p.seg[s].OW : c_OW;
      c_SH = in ? p.seg[s].SH : c_SH;
      c_SW = in ? p.seg[s].SW : c_SW;
      c_end = in ? ((s + 1 < p.n_seg) ? p.seg[s + 1].row_begin : 0x7fffffff) : c_end;
    }
    const int local = m < p.M ? m - rbeg : 0;
    const int hw = c_OH * c_OW;
    int rem;
    const int n = div_small(local, hw, __frcp_rn((float)hw), &rem);
    r_y = div_small(rem, c_OW, __frcp_rn((float)c_OW), &r_x);
    r_img = sb + n * c_SH * c_SW;
  };
  decode(m_cur);
  const int n_wraps = p.max_wraps;
  int q_next = blk_past;  // SP: the listed block of the step after the one being loaded
  if (SP) q_next = (s_idx + 1 < s_end) ? g_list[1 + s_idx + 1] : blk_past;

  auto load_step = [&]() {
    const int m = m_cur;
    const bool in_rng = m < m_end;
    const int sy = r_y * p.stride + ty - p.pad_t, sx = r_x * p.stride + tx - p.pad_l;
    const bool ok = in_rng && ((unsigned)sy < (unsigned)c_SH) && ((unsigned)sx < (unsigned)c_SW);
    int xo = ((r_img + sy * c_SW + sx) * p.ld_src + ci0) * ES + CB * q8;
    xo = ok ? xo : PP_BUF_OOB;
#pragma unroll
    for (int j = 0; j < QA; ++j) {
      ra[j] = buf_load16(rs_x0, xo, 8 * CB * j);
      if (AP) ral[j] = buf_load16(rs_x1, xo, 8 * CB * j);
    }
    const int dyo = (m * p.ld_dy + n0) * ES + CB * q8;
#pragma unroll
    for (int j = 0; j < QB; ++j) {
      const bool okb = in_rng && (n0 + CH * (q8 + 8 * j) < p.ld_dy);
      const int o = okb ? dyo : PP_BUF_OOB;
      rb[j] = buf_load16(rs_d0, o, 8 * CB * j);
      if (AP) rbl[j] = buf_load16(rs_d1, o, 8 * CB * j);
    }
  };
  auto next_row = [&]() {  // m_cur += 32
    if (SP) {  // jump to the next listed block: full decode (two reciprocal divisions per step).  The list entry was fetched one
               // step ahead (q_next): a dependent global load in front of the operand loads cost ~1 us per step
      ++s_idx;
      m_cur = q_next * BK + prow;
      q_next = (s_idx + 1 < s_end) ? g_list[1 + s_idx + 1] : blk_past;
      decode(m_cur);
      return;
    }
    m_cur += BK;
    if (__builtin_amdgcn_ballot_w64(m_cur >= c_end) != 0) {
      decode(m_cur);
    } else {
      r_x += BK;
      for (int i = 0; i < n_wraps; ++i) {
        const bool w = r_x >= c_OW;
        r_x -= w ? c_OW : 0;
        r_y += w ? 1 : 0;
      }
      const bool wy = r_y >= c_OH;  // (32 consecutive cells never span more than one image boundary: OH * OW >= 32 is host-checked)
      r_y -= wy ? c_OH : 0;
      r_img += wy ? c_SH * c_SW : 0;
    }
  };
  auto split_step = [&](auto with_bias) {  // conversion (f32 path) and the bias partial sums: VALU only, under the MFMAs
    constexpr bool WB = decltype(with_bias)::value;
    const float bmask = 1.f;
    if (AP) {
      if (!WB) return;
#pragma unroll
      for (int j = 0; j < QB; ++j) {  // dy = hi + lo (2^-17)
        const unsigned int hw4[4] = {rb[j].x, rb[j].y, rb[j].z, rb[j].w}, lw4[4] = {rbl[j].x, rbl[j].y, rbl[j].z, rbl[j].w};
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) fmt_value2(hw4[e], lw4[e], &v[2 * e], &v[2 * e + 1]);
        bsum[2 * j].x = fmaf(v[0], bmask, bsum[2 * j].x); bsum[2 * j].y = fmaf(v[1], bmask, bsum[2 * j].y);
        bsum[2 * j].z = fmaf(v[2], bmask, bsum[2 * j].z); bsum[2 * j].w = fmaf(v[3], bmask, bsum[2 * j].w);
        bsum[2 * j + 1].x = fmaf(v[4], bmask, bsum[2 * j + 1].x); bsum[2 * j + 1].y = fmaf(v[5], bmask, bsum[2 * j + 1].y);
        bsum[2 * j + 1].z = fmaf(v[6], bmask, bsum[2 * j + 1].z); bsum[2 * j + 1].w = fmaf(v[7], bmask, bsum[2 * j + 1].w);
      }
    } else {
#pragma unroll
      for (int j = 0; j < QA; ++j) split4(*reinterpret_cast<const float4*>(&ra[j]), &sah[j], &sal[j]);
#pragma unroll
      for (int j = 0; j < QB; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(&rb[j]);
        split4(v, &sbh[j], &sbl[j]);
        if (WB) { bsum[j].x += v.x; bsum[j].y += v.y; bsum[j].z += v.z; bsum[j].w += v.w; }
      }
    }
  };
  auto store_step = [&]() {
#pragma unroll
    for (int j = 0; j < QA; ++j) {
      const int off = prow * PA + CH * (q8 + 8 * j);
      if (AP) {
        *reinterpret_cast<uint4*>(Xhi + off) = ra[j];
        *reinterpret_cast<uint4*>(Xlo + off) = ral[j];
      } else {
        *reinterpret_cast<uint2*>(Xhi + off) = sah[j];
        *reinterpret_cast<uint2*>(Xlo + off) = sal[j];
      }
    }
#pragma unroll
    for (int j = 0; j < QB; ++j) {
      const int off = prow * PB + CH * (q8 + 8 * j);
      if (AP) {
        *reinterpret_cast<uint4*>(Ghi + off) = rb[j];
        *reinterpret_cast<uint4*>(Glo + off) = rbl[j];
      } else {
        *reinterpret_cast<uint2*>(Ghi + off) = sbh[j];
        *reinterpret_cast<uint2*>(Glo + off) = sbl[j];
      }
    }
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int c = 0; c < TN; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;

  // transposed-read lane roles (16-lane groups): group g -> columns 16*(g&1).., pixel half h = g>>1
  const int grp = lane >> 4, gi = lane & 15, gq = gi >> 2, gp = gi & 3;
  const int cbase = 16 * (grp & 1), hh = grp >> 1;
  const int il = lane & 31, h = lane >> 5;

  auto k_loop = [&](auto with_bias) {
    load_step();  // (n_steps == 0: every row is out of range -> zeros)
    split_step(with_bias);
    store_step();
    __syncthreads();
    for (int step = 0; step < n_steps; ++step) {
      next_row();
      load_step();  // past the last step m >= m_end: zeros, never stored
      __builtin_amdgcn_sched_barrier(0);
      wgrad_step<TM, TN>(acc, Xhi, Xlo, Ghi, Glo, PA, PB, wm * 32 * TM + cbase + 4 * gp, wn * 32 * TN + cbase + 4 * gp, hh, gq);
      split_step(with_bias);
      __syncthreads();
      store_step();
      __syncthreads();
    }
  };
  if (do_bias) k_loop(std::true_type{});
  else k_loop(std::false_type{});

  // Reduction over the row splits.  With a scratch buffer (pp_ctx_set_workspace): split s writes its partial tile -- plain
  // stores, every column of the tile below ld_w, zeros past Cout -- into slice s, a full-size copy of dW (+ one bias row), and
  // wgrad_finish_kernel adds the slices in a fixed order: deterministic, and the partial sums leave the chip at store speed
  // instead of the ~1.3 TB/s of float atomics (MI355X_MICROARCH.md: they execute at the memory side).  Without it: atomics.
  float* const slice = g_ws ? g_ws + (long long)split * ws_slice : nullptr;
#pragma unroll
  for (int a = 0; a < TM; ++a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = ci0 + wm * 32 * TM + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      const long long row = (long long)(tap * p.Cin + ci) * p.ld_w;
#pragma unroll
      for (int c = 0; c < TN; ++c) {
        const int co = n0 + wn * 32 * TN + c * 32 + il;
        if (slice) {
          if (co < p.ld_w) slice[row + co] = co < p.Cout ? acc[a][c][r] * inv_g : 0.f;
        } else if (co < p.Cout) {
          atomicAdd(g_dw + row + co, acc[a][c][r] * inv_g);
        }
      }
    }
  }
  if (do_bias) {
    // 32 threads (one per pixel row of the step) hold partial sums of the same channels: reduce through LDS
    float* red = reinterpret_cast<float*>(smem);  // [32][BN] floats <= LDS size
    __syncthreads();
    if (AP) {
#pragma unroll
      for (int j = 0; j < QB; ++j) {
        *reinterpret_cast<float4*>(red + prow * BN + 8 * (q8 + 8 * j)) = bsum[2 * j];
        *reinterpret_cast<float4*>(red + prow * BN + 8 * (q8 + 8 * j) + 4) = bsum[2 * j + 1];
      }
    } else {
#pragma unroll
      for (int j = 0; j < QB; ++j) *reinterpret_cast<float4*>(red + prow * BN + 4 * (q8 + 8 * j)) = bsum[j];
    }
    __syncthreads();
    if (tid < BN) {
      float s = 0.f;
#pragma unroll 8
      for (int r = 0; r < 32; ++r) s += red[r * BN + tid];
      if (slice) {
        if (n0 + tid < p.ld_w) slice[ws_slice - p.ld_w + n0 + tid] = n0 + tid < p.Cout ? s * inv_g : 0.f;  // the bias row closes the slice
      } else if (n0 + tid < p.Cout) {
        atomicAdd(g_dbias + n0 + tid, s * inv_g);
      }
    }
  }
}

// dw += sum_s slice_s (fixed order), dbias += the slices' last row; n4 = float4 groups of one slice (dW + the bias row)
__global__ void wgrad_finish_kernel(long long n4_dw, int ld4, int splits, long long ws_slice4, const float4* __restrict__ ws, float4* __restrict__ dw,
                                    float4* __restrict__ dbias) {
  const long long total = n4_dw + (dbias ? ld4 : 0);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const bool is_bias = i >= n4_dw;
    const long long src = is_bias ? ws_slice4 - ld4 + (i - n4_dw) : i;
    float4 v = ws[src];
    for (int s = 1; s < splits; ++s) {
      const float4 q = ws[src + s * ws_slice4];
      v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    }
    float4* dst = is_bias ? dbias + (i - n4_dw) : dw + i;
    float4 o = *dst;
    o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
    *dst = o;
  }
}

// the launches of one weight-gradient plan (conv_plan.h: pp_plan_wgrad) on its tile
template <int TM, int TN>
static void launch_wgrad3(hipStream_t st, const Wgrad3Params& p, const PpWgradPlan& pl, const float* x, const float* dy, const void* xhi,
                          const void* xlo, const void* dhi, const void* dlo, float* dw, float* dbias, const int* list, float* ctx_ws) {
  const dim3 grid(pl.grid), wg(256);
  const unsigned x_bytes = (unsigned)(p.src_rows * (long long)p.ld_src * 4), d_bytes = (unsigned)((long long)p.M * p.ld_dy * 4);  // f32 or packed planes
  float* const ws = pl.finish_blocks ? ctx_ws : nullptr;  // (a single split adds its tile straight into dW)
  auto go = [&](auto ap, auto sp) {  // operands as planes (AP) or f32; SP: over the listed blocks
    constexpr bool AP = decltype(ap)::value, SP = decltype(sp)::value;
    if (pl.family != PP_WGRAD3)
      hipLaunchKernelGGL((wgrad3f_kernel<TM, TN, AP, SP>), grid, wg, 0, st, p, AP ? xhi : (const void*)x, AP ? xlo : nullptr, x_bytes,
                         AP ? dhi : (const void*)dy, AP ? dlo : nullptr, d_bytes, dw, dbias, SP ? list : (const int*)nullptr, ws, pl.ws_slice);
    else if constexpr (!SP)
      hipLaunchKernelGGL((wgrad3_kernel<TM, TN, AP>), grid, wg, 0, st, p, x, dy, (const uint4*)(AP ? xhi : nullptr), (const uint4*)(AP ? xlo : nullptr),
                         (const uint4*)(AP ? dhi : nullptr), (const uint4*)(AP ? dlo : nullptr), dw, dbias);
  };
  const std::true_type yes{};
  const std::false_type no{};
  switch (pl.family) {
    case PP_WGRAD3F_PLANES_LIST: go(yes, yes); break;
    case PP_WGRAD3F_PLANES: go(yes, no); break;
    case PP_WGRAD3F_F32_LIST: go(no, yes); break;
    case PP_WGRAD3F_F32: go(no, no); break;
    default:  // PP_WGRAD3
      if (xhi) go(yes, no);
      else go(no, no);
  }
  if (ws)
    hipLaunchKernelGGL(wgrad_finish_kernel, dim3(pl.finish_blocks), wg, 0, st, (pl.ws_slice - p.ld_w) / 4, p.ld_w / 4, pl.splits, pl.ws_slice / 4,
                       (const float4*)ws, (float4*)dw, (float4*)dbias);
}

}  // namespace

void PP_API(pp3_launch_wgrad)(hipStream_t st, const Wgrad3Params& p, const PpWgradPlan& pl, const float* x, const float* dy, const void* xhi,
                              const void* xlo, const void* dhi, const void* dlo, float* dw, float* dbias, const int* list, float* ctx_ws) {
  if (pl.tm == 2 && pl.tn == 2) launch_wgrad3<2, 2>(st, p, pl, x, dy, xhi, xlo, dhi, dlo, dw, dbias, list, ctx_ws);
  else if (pl.tm == 2) launch_wgrad3<2, 1>(st, p, pl, x, dy, xhi, xlo, dhi, dlo, dw, dbias, list, ctx_ws);
  else if (pl.tn == 2) launch_wgrad3<1, 2>(st, p, pl, x, dy, xhi, xlo, dhi, dlo, dw, dbias, list, ctx_ws);
  else launch_wgrad3<1, 1>(st, p, pl, x, dy, xhi, xlo, dhi, dlo, dw, dbias, list, ctx_ws);
}
