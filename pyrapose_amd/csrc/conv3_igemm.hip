// The forward / data-gradient kernels of the plane-format convolution family -- igemm3, igemm3f (plain, parity-class, row-list and
// merged stride-2 forms), igemm3x -- with their finishing, fill and dilation kernels and the launch code that runs a plan
// (conv_plan.h) on them; the launchers are declared in conv3.h.  The arithmetic of the family is described at the head of conv3.hip.
#include "conv3_unit.h"
#include "conv3.h"
#include "conv4.h"

#ifndef PP_EPI_GF
#define PP_EPI_GF 4  // output rows in flight per thread in igemm3f's epilogue (8 measured in round 4: see DESIGN.md)
#endif

namespace {

template <int TM, int TN, bool AP, bool OP>
__global__ __launch_bounds__(256, (TM * TN >= 8) ? 2 : ((TM * TN == 4) ? 3 : 4)) void igemm3_kernel(
    const IgemmParams p, const float* __restrict__ g_src, const uint4* __restrict__ g_ahi, const uint4* __restrict__ g_alo,
    const uint4* __restrict__ g_whi, const uint4* __restrict__ g_wlo,
    const float* __restrict__ g_bias, const float* __restrict__ g_addend, const float* __restrict__ g_mask,
    float* __restrict__ g_out, uint2* __restrict__ g_ohi, uint2* __restrict__ g_olo, int w_rows, int w_ld8) {
  constexpr int BM = 64 * TM, BN = 64 * TN, BK = 32, NO = BK / 8;
  constexpr int SMEM_U4 = 2 * NO * (BM + BN);
  __shared__ __attribute__((aligned(16))) uint4 smem[SMEM_U4];
  uint4* Ahi = smem;
  uint4* Alo = Ahi + NO * BM;
  uint4* Bhi = Alo + NO * BM;
  uint4* Blo = Bhi + NO * BN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lb = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int tile_n = lb % p.n_tiles_n, tile_m = lb / p.n_tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  // staging threads: 4 per row (one k-octet = 8 channels each), rows r0 + 64*i
  const int oct = tid & 3, r0 = tid >> 2;
  RowPos rows[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) rows[i] = decode_row(p, m0 + r0 + 64 * i);
  long long a_off[TM];
  bool a_ok[TM];

  const int n_taps = p.kh * p.kw;
  const int n_steps = n_taps * (p.Cred / BK);

  float4 ra[TM][2];
  uint4 rah[TM], ral[TM];
  uint4 rbh[TN], rbl[TN];
  int tap = 0, ty = 0, tx = 0, red0 = 0;

  auto set_tap = [&]() {
#pragma unroll
    for (int i = 0; i < TM; ++i) a_ok[i] = tap_offset(p, rows[i], ty, tx, &a_off[i]);
  };
  auto load_step = [&]() {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      if (AP) {
        if (a_ok[i]) {
          const long long o8 = 2 * (((a_off[i] + red0) >> 3) + oct);  // packed planes: 32-byte groups
          rah[i] = g_ahi[o8];
          ral[i] = g_alo[o8];
        } else {
          rah[i] = make_uint4(0u, 0u, 0u, 0u);
          ral[i] = make_uint4(0u, 0u, 0u, 0u);
        }
      } else if (a_ok[i]) {
        const float4* s4 = reinterpret_cast<const float4*>(g_src + a_off[i] + red0 + 8 * oct);
        ra[i][0] = s4[0];
        ra[i][1] = s4[1];
      } else {
        ra[i][0] = make_float4(0.f, 0.f, 0.f, 0.f);
        ra[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      const int n = n0 + r0 + 64 * i;
      if (n < w_rows) {
        const long long off = ((long long)tap * w_rows + n) * w_ld8 + (red0 >> 3) + oct;
        rbh[i] = g_whi[off];
        rbl[i] = g_wlo[off];
      } else {
        rbh[i] = make_uint4(0u, 0u, 0u, 0u);
        rbl[i] = make_uint4(0u, 0u, 0u, 0u);
      }
    }
  };
  auto advance = [&]() {
    red0 += BK;
    if (red0 >= p.Cred) {
      red0 = 0;
      ++tap;
      ++tx;
      if (tx == p.kw) { tx = 0; ++ty; }
      set_tap();
    }
  };
  auto store_step = [&]() {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      uint4 hi, lo;
      if (AP) {
        hi = rah[i];
        lo = ral[i];
      } else {
        split8(ra[i][0], ra[i][1], &hi, &lo);
      }
      const int slot = oct * BM + ((r0 + 64 * i + 2 * oct) & (BM - 1));
      Ahi[slot] = hi;
      Alo[slot] = lo;
    }
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      const int slot = oct * BN + ((r0 + 64 * i + 2 * oct) & (BN - 1));
      Bhi[slot] = rbh[i];
      Blo[slot] = rbl[i];
    }
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int il = lane & 31, h = lane >> 5;

  set_tap();
  load_step();
  store_step();
  __syncthreads();

  // Measured alternatives that were NOT kept: double-buffered LDS with one barrier per step (64 KB per workgroup,
  // occupancy 3 -> 2: 15-20 % slower); weights streamed by LDS-DMA (global_load_lds_dwordx4, swizzled source,
  // double-buffered B stage): correct but 2-5 % slower -- the DMA issue cost replaces the ds_write cost.
  for (int step = 0; step < n_steps; ++step) {
    const bool more = step + 1 < n_steps;
    if (more) {
      advance();
      load_step();  // in flight under the MFMAs below
    }
    mma_step<TM, TN, BM, BN, 0>(acc, Ahi, Alo, Bhi, Blo, wm * 32 * TM + il, wn * 32 * TN + il, h);
    __syncthreads();  // every wave has read this step's tiles
    if (more) {
      store_step();
      __syncthreads();
    }
  }

  epilogue3<TM, TN, OP>(p, acc, smem, m0, n0, tid, wm, wn, il, h, g_bias, g_addend, g_mask, g_out, g_ohi, g_olo);
}

// ---- igemm3f: the same tile and LDS image with a branch-free, 32-bit-addressed main loop ----
// For gathers that are linear in the tap (div == 1: forward at any stride, bwd-data at stride 1).  Per staged row the
// kernel keeps a byte offset of tap (0,0), the row pitch of its level and a validity bit per tap; every step's
// operand addresses are then 4 VALU per row (mad + add + bit test + select) and the loads are raw buffer loads,
// whose out-of-range offsets return zeros -- padding taps and rows past M need no branch, so the whole k-loop body
// is ONE basic block that the scheduler can interleave under the MFMAs.  Buffers must stay below 2 GiB
// (host-checked; larger tensors take igemm3_kernel).
// Measured and NOT kept (tools/conv_bench.py --shape r3 = exactly three rounds of workgroups, 128x128 tile): a 64-deep k-step
// (twice the MFMAs per barrier pair, 2 workgroups/CU) and register double-buffering of the staged tiles (loads issued two
// steps ahead, 190 VGPRs, 2 workgroups/CU) both land on the same 340-355 TFLOP/s as this loop; dependent MFMAs on one
// accumulator issue back to back at full rate (tools/ubench/mfma_dep.hip).  Ablations of this loop: without global loads
// +30 %, without the f32->bf16 conversion +17 %, with the gathered operand loaded for one tap in nine +12 %, MFMA +
// fragment reads alone 530 TFLOP/s: the staging of the SAME activation rows for each of the nine taps is what is left.
// Measured and NOT kept: walking the grid column-tile-major per XCD (one column tile's 2.4 MB of weight planes resident in
// each 4 MiB L2, activations re-read by four XCDs): 2-5 % slower on the head shapes than the row-tile-major order -- the
// 3x3 gather re-reads its activation rows nine times, so keeping THEM in L2 matters more than the weights.
// Measured and NOT kept: the same loop on v_mfma_f32_16x16x32_bf16 (48 instead of 24 MFMAs per step, lane = (row, octet)
// staging map, un-rotated image): bit-identical results, 20 % slower on every head shape (255-295 vs 325-355 TFLOP/s).
// RL (row list): the launch computes only the 32-row output blocks of a list (g_rl[0] = count, g_rl[1 ..] ascending block
// indices; pp_conv_opts.skip_flags: the blocks of the data gradient that a non-zero of dy can reach), four (two) blocks
// to a tile; the grid is sized for the dense case and workgroups past the end of the list leave at once.  Rows keep their
// own gather offsets (this loop never assumed that the rows of a tile are consecutive); rl_fill_kernel writes the rest.
// MG (merged stride-2 data gradient, igemm3m_kernel): the workgroup is number `bid` of the `n_wg_in` workgroups of ITS parity
// class, p holds that class's geometry, and a class may have no taps: no step is staged or run, the accumulators stay zero and
// the epilogue writes mask?(addend or 0).
template <int TM, int TN, bool AP, bool OP, bool SC, bool RL, bool MG>
__device__ __forceinline__ void igemm3f_body(
    const IgemmParams& p, const int bid, const int n_wg_in, const void* __restrict__ g_a0, const void* __restrict__ g_a1, unsigned a_bytes,
    const void* __restrict__ g_whi, const void* __restrict__ g_wlo, unsigned w_bytes,
    const float* __restrict__ g_bias, const float* __restrict__ g_addend, const float* __restrict__ g_mask,
    float* __restrict__ g_out, uint2* __restrict__ g_ohi, uint2* __restrict__ g_olo, int w_rows, int w_ld8, int splits,
    float* __restrict__ g_ws, const int* __restrict__ g_rl, const unsigned char* __restrict__ g_srcflags) {
  constexpr int BM = 64 * TM, BN = 64 * TN, BK = 32, NO = BK / 8;
  constexpr int SMEM_U4 = 2 * NO * (BM + BN);
  constexpr int ES = 4;  // bytes per gathered element: f32, or packed planes (hi at the group's offset, lo 16 bytes behind = rs_a1)
  __shared__ __attribute__((aligned(16))) uint4 smem[SMEM_U4];
  uint4* Ahi = smem;
  uint4* Alo = Ahi + NO * BM;
  uint4* Bhi = Alo + NO * BM;
  uint4* Blo = Bhi + NO * BN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  int n_wg = n_wg_in;
  if (RL) {  // the grid is sized for the dense case: only the first ceil(count / blocks per tile) x n_tiles_n workgroups work,
             // and the XCD remap runs over THEM (over the whole grid the listed tiles would all land on the first XCDs)
    n_wg = ((g_rl[0] + BM / 32 - 1) / (BM / 32)) * p.n_tiles_n * splits;
    if (bid >= n_wg) return;  // workgroup-uniform, before any barrier
  }
  // (MG: workgroups bid = b (mod 8) of one class share an XCD -- the class's first workgroup only shifts WHICH one)
  const int lbs = xcd_remap(bid, n_wg);
  const int split = lbs % splits, lb = lbs / splits;  // split-K: `splits` workgroups share one output tile
  const int tile_n = lb % p.n_tiles_n, tile_m = lb / p.n_tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  int rl_blk[BM / 32];  // RL: first row of each listed block of this tile
  if (RL) {
    const int count = g_rl[0];
#pragma unroll
    for (int j = 0; j < BM / 32; ++j) {
      const int e = tile_m * (BM / 32) + j;
      rl_blk[j] = e < count ? g_rl[1 + e] * 32 : ((p.M + 31) & ~31);
    }
  }
  const int oct = tid & 3, r0 = tid >> 2;
  const int n_taps = p.kh * p.kw;
  const int steps_per_tap = p.Cred / BK;
  const int all_steps = n_taps * steps_per_tap;
  const int s_begin = (int)((long long)all_steps * split / splits), s_end = (int)((long long)all_steps * (split + 1) / splits);

  const __amdgpu_buffer_rsrc_t rs_a0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g_a0), 0, a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_a1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(AP ? g_a1 : g_a0), 0, AP ? a_bytes - 16 : a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_wh = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g_whi), 0, w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_wl = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g_wlo), 0, w_bytes, 0x00020000);

  // per staged row: byte offset at tap (0,0), pitch of one tap row, validity bit per tap
  int a_base[TM], a_pitch[TM];
  unsigned a_valid[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int t_row = r0 + 64 * i;
    const RowPos r = decode_row(p, RL ? rl_blk[t_row >> 5] + (t_row & 31) : m0 + t_row);
    a_base[i] = ((r.rowbase + r.ybase * r.SW + r.xbase) * p.ld_src + 8 * oct) * ES;
    a_pitch[i] = p.tsign * r.SW * p.ld_src * ES;
    unsigned v = 0;
    int t = 0;
    for (int ty = 0; ty < p.kh; ++ty)
      for (int tx = 0; tx < p.kw; ++tx, ++t) {
        const int sy = r.ybase + ty * p.tsign, sx = r.xbase + tx * p.tsign;
        bool ok = r.ok && (unsigned)sy < (unsigned)r.SH && (unsigned)sx < (unsigned)r.SW;
        // RL with the flags of the gathered tensor (sparse bwd-data): a source row outside the flagged 32-row blocks IS zero by
        // the meaning of the flags -- it is not fetched, so a producer may leave such rows unwritten (pp_conv_opts.lazy_out)
        if (RL && g_srcflags && ok) ok = g_srcflags[(r.rowbase + sy * r.SW + sx) >> 5] != 0;
        if (ok) v |= 1u << t;
      }
    a_valid[i] = v;
  }
  const int x_pitch = p.tsign * p.ld_src * ES;
  int b_base[TN];
#pragma unroll
  for (int i = 0; i < TN; ++i) {
    const int n = n0 + r0 + 64 * i;
    b_base[i] = n < w_rows ? (n * w_ld8 + oct) * 16 : PP_BUF_OOB;
  }
  const int b_tap = w_rows * w_ld8 * 16;

  float4 ra[TM][2];
  uint4 rah[TM], ral[TM];
  uint4 rbh[TN], rbl[TN];
  int tap = s_begin / steps_per_tap, red0 = (s_begin - tap * steps_per_tap) * BK;
  int ty = tap / (MG ? max(p.kw, 1) : p.kw), tx = tap - ty * p.kw;  // (MG: a class without taps has kw == 0)

  auto load_step = [&]() {
    const int a_uni = tx * x_pitch + red0 * ES;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      int vo = a_base[i] + __mul24(ty, a_pitch[i]) + a_uni;
      vo = ((a_valid[i] >> tap) & 1u) ? vo : PP_BUF_OOB;
      if (AP) {
        rah[i] = buf_load16(rs_a0, vo, 0);
        ral[i] = buf_load16(rs_a1, vo, 0);
      } else {
        const uint4 q0 = buf_load16(rs_a0, vo, 0), q1 = buf_load16(rs_a0, vo + 16, 0);
        ra[i][0] = *reinterpret_cast<const float4*>(&q0);
        ra[i][1] = *reinterpret_cast<const float4*>(&q1);
      }
    }
    const int b_uni = ((p.w_ty0 + p.w_tstep * ty) * p.w_kw + p.w_tx0 + p.w_tstep * tx) * b_tap + (red0 >> 3) * 16;
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      rbh[i] = buf_load16(rs_wh, b_base[i], b_uni);
      rbl[i] = buf_load16(rs_wl, b_base[i], b_uni);
    }
  };
  auto advance = [&](bool more) {  // uniform, branch-free; past the last step it rewinds to step 0 (a harmless re-load)
    red0 += BK;
    const bool wrap = red0 >= p.Cred;
    red0 = wrap ? 0 : red0;
    tap += wrap ? 1 : 0;
    tx += wrap ? 1 : 0;
    const bool wx = tx == p.kw;
    tx = wx ? 0 : tx;
    ty += wx ? 1 : 0;
    red0 = more ? red0 : 0;
    tap = more ? tap : 0;
    tx = more ? tx : 0;
    ty = more ? ty : 0;
  };
  auto split_step = [&]() {
    if (!AP) {
#pragma unroll
      for (int i = 0; i < TM; ++i) split8(ra[i][0], ra[i][1], &rah[i], &ral[i]);
    }
  };
  auto store_step = [&]() {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int slot = oct * BM + ((r0 + 64 * i + 2 * oct) & (BM - 1));
      Ahi[slot] = rah[i];
      Alo[slot] = ral[i];
    }
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      const int slot = oct * BN + ((r0 + 64 * i + 2 * oct) & (BN - 1));
      Bhi[slot] = rbh[i];
      Blo[slot] = rbl[i];
    }
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int il = lane & 31, h = lane >> 5;

  if (!MG || s_begin < s_end) {  // (workgroup-uniform)
    load_step();
    split_step();
    store_step();
  }
  __syncthreads();

  for (int step = s_begin; step < s_end; ++step) {
    advance(step + 1 < s_end);
    load_step();  // in flight under the MFMAs below
    // (left alone the scheduler sinks the loads below the MFMAs, or pulls the conversion of the loaded tile -- and
    // with it the wait for the loads -- up to the first MFMA: pin loads | first half of the MFMAs | rest + conversion)
    __builtin_amdgcn_sched_barrier(0);
    mma_step<TM, TN, BM, BN, 2>(acc, Ahi, Alo, Bhi, Blo, wm * 32 * TM + il, wn * 32 * TN + il, h);
    split_step();     // conversion VALU issues while this wave's MFMAs drain
    __syncthreads();  // every wave has read this step's tiles
    store_step();
    __syncthreads();
  }
  if (splits > 1) {  // partial sums only (slice `split` of the scratch): splitk_finish_kernel sums the slices in a fixed
                     // order and applies the epilogue -> deterministic, no atomics, nothing to zero
    // (RL: slice rows are COMPACT -- list position * 32 + row in the block, i.e. m0 + tile row -- and every row of a listed
    // block is written, in range or not: rl_splitk_finish_kernel reads them by list position)
    float* slice = g_ws + (long long)split * (RL ? (((long long)p.M + 31) & ~31ll) : (long long)p.M) * p.ld_out;
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int trow = wm * 32 * TM + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const int m = m0 + trow;
        const bool row_ok = RL ? (rl_blk[trow >> 5] < p.M) : (m < p.M);
#pragma unroll
        for (int b = 0; b < TN; ++b) {
          const int co = n0 + wn * 32 * TN + b * 32 + il;
          if (row_ok && co < ((p.Nout + 3) & ~3)) slice[(long long)m * p.ld_out + co] = acc[a][b][r];
        }
      }
    return;
  }
  epilogue3<TM, TN, OP, PP_EPI_GF, SC, false, RL>(p, acc, smem, m0, n0, tid, wm, wn, il, h, g_bias, g_addend, g_mask, g_out, g_ohi, g_olo, rl_blk);
}

template <int TM, int TN, bool AP, bool OP, bool SC = false, bool RL = false>
__global__ __launch_bounds__(256, (TM * TN >= 8) ? 2 : ((TM * TN == 4) ? 3 : 4)) void igemm3f_kernel(
    const IgemmParams p, const void* __restrict__ g_a0, const void* __restrict__ g_a1, unsigned a_bytes,
    const void* __restrict__ g_whi, const void* __restrict__ g_wlo, unsigned w_bytes,
    const float* __restrict__ g_bias, const float* __restrict__ g_addend, const float* __restrict__ g_mask,
    float* __restrict__ g_out, uint2* __restrict__ g_ohi, uint2* __restrict__ g_olo, int w_rows, int w_ld8, int splits,
    float* __restrict__ g_ws, const int* __restrict__ g_rl = nullptr, const unsigned char* __restrict__ g_srcflags = nullptr) {
  igemm3f_body<TM, TN, AP, OP, SC, RL, false>(p, (int)blockIdx.x, (int)gridDim.x, g_a0, g_a1, a_bytes, g_whi, g_wlo, w_bytes, g_bias, g_addend,
                                              g_mask, g_out, g_ohi, g_olo, w_rows, w_ld8, splits, g_ws, g_rl, g_srcflags);
}

// ---- igemm3m: the stride-2 data gradient, all parity classes in one launch (pp_conv2d_nhwc_bwd_data_s2_bf16x3) ----
// The grid is the classes' tile grids one behind the other (conv_plan.h: pp_s2_merge, heaviest class first).  A workgroup
// compares its index with at most three prefix sums -- workgroup-uniform, scalar selects, no division --, takes that class's
// geometry into its copy of the parameters and runs igemm3f's body on it: every tile runs the products the per-class launch
// runs, in the same order, so the results are bit-identical to pp_conv2d_nhwc_bwd_data_bf16x3; a class without taps writes what
// class_fill_kernel writes.  p: the whole gradient with the fields all classes share (sc_on, sc_H, sc_W, w_tstep = 2, div = 1).
template <int TM, int TN, bool AP, bool OP>
__global__ __launch_bounds__(256, (TM * TN >= 8) ? 2 : ((TM * TN == 4) ? 3 : 4)) void igemm3m_kernel(
    const IgemmParams p0, const PpS2Merged g, const void* __restrict__ g_a0, const void* __restrict__ g_a1, unsigned a_bytes,
    const void* __restrict__ g_whi, const void* __restrict__ g_wlo, unsigned w_bytes, const float* __restrict__ g_addend,
    const float* __restrict__ g_mask, float* __restrict__ g_out, uint2* __restrict__ g_ohi, uint2* __restrict__ g_olo, int w_rows, int w_ld8) {
  const int bid = (int)blockIdx.x;
  PpS2Class c = g.c[0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (j < g.n_cls && bid >= g.c[j].blk_begin) c = g.c[j];
  IgemmParams p = p0;
  p.n_seg = 1;  // (host-checked; as a constant it removes the level loop of decode_row, whose indexing would keep this copy in memory)
  igemm_set_class(p, c);
  igemm3f_body<TM, TN, AP, OP, true, false, true>(p, bid - c.blk_begin, c.tiles, g_a0, g_a1, a_bytes, g_whi, g_wlo, w_bytes, nullptr, g_addend, g_mask,
                                                  g_out, g_ohi, g_olo, w_rows, w_ld8, 1, nullptr, nullptr, nullptr);
}

// ---- igemm3x: 3-wide stride-1 "same" convolutions with the gathered tile shared by the three taps of a kernel row ----
// For a fixed kernel row ty the source pixel of output row m at tap tx is (m + dy * W(m)) + dx with dx = off_x + tx * tsign
// in {-1, 0, 1}: the tile of tap dx is the tile of dx = 0 shifted by one row.  The workgroup stages its BM rows once per
// (ty, 32-channel chunk) and the three taps read their fragments at row offsets -1, 0, +1; so that every output row finds
// both neighbours inside the tile, consecutive tiles overlap by two rows: a tile covers output rows m0 .. m0 + BM - 1 but
// only writes the BM - 2 inner ones (1.6 % of the MFMAs are spent on the two edge rows).  A row shifted across an
// image-row / image / pyramid-level boundary lands on the wrong pixel exactly where the tap is padding: the per-lane
// tap-validity bit zeroes that fragment.  Global loads, f32->bf16 conversions and LDS writes of the gathered operand drop
// to a third.  Loop order: ty, channel chunk, tx (unrolled: the body of each tx is one basic block).
// Conditions (host-checked): kw == 3, stride 1, source space == enumerated space (SH == OH, SW == OW, same row offsets),
// f32 source, no planes / scatter.
// Where the time went before the iglp_opt hint below (profiles/r01_pmc_stalls.txt, 128x128; 65 % MFMA-busy with it): MFMA pipe 58 % busy, VALU 19 % (8 % under an MFMA), LDS unit
// 34 %, no bank conflicts; for 31 % of the cycles all three resident waves of a SIMD wait (barriers, LDS / global
// latency).  Tried against that: a double-buffered weight tile (one barrier per tap instead of two, 48 KB of LDS): the
// kernel alone gains 1 %, the training step loses 1 % (less room for the other lane's workgroups on the CU) -- not kept;
// s_setprio 2 / 0 around the MFMA bursts (the hipBLASLt habit): 1 % slower alone and in the step.
// CAP: the bf16 (hi, lo) split of the gathered f32 operand is also written out ([rows][ld_src] planes, the geometry of
// pp_split_planes_bf16x3): for the centre kernel row (dy = 0: the staged rows are the tile's own rows; the BM - 2 inner
// rows of all tiles cover every row once) the workgroups store the registers they have just converted, the output-channel
// tiles of one row tile taking turns over the channel chunks.  The weight-gradient launch of the same layer then reads both operands pre-split (pp_conv_opts.capture_hi / capture_lo).
// AP: the gathered operand is stored as bf16 (hi, lo) planes (g_a = hi, g_a1 = lo; ld_src % 8 == 0): the staging threads move
// 16 B of each plane per row and chunk -- the same bytes as the two f32 quads -- and nothing is converted in the loop.
// OP: the output tile is written as planes (g_ohi / g_olo; also as f32 when g_out != NULL).
template <int TM, int TN, bool CAP, bool AP = false, bool OP = false>
__global__ __launch_bounds__(256, (TM * TN >= 8) ? 2 : ((TM * TN == 4) ? 3 : 4)) void igemm3x_kernel(
    const IgemmParams p, const void* __restrict__ g_a, const void* __restrict__ g_a1, unsigned a_bytes, const void* __restrict__ g_whi,
    const void* __restrict__ g_wlo, unsigned w_bytes, const float* __restrict__ g_bias, const float* __restrict__ g_addend,
    const float* __restrict__ g_mask, float* __restrict__ g_out, uint2* __restrict__ g_ohi, uint2* __restrict__ g_olo, int w_rows, int w_ld8,
    int splits, float* __restrict__ g_ws, void* __restrict__ g_chi, void* __restrict__ g_clo, const unsigned char* __restrict__ g_flags,
    int skip_halo) {
  static_assert(!(CAP && AP), "split capture is for f32 operands");
  constexpr int ES = 4;  // bytes per gathered element: f32, or packed planes (hi at the group's offset, lo 16 bytes behind = rs_a1)
  constexpr int BM = 64 * TM, BN = 64 * TN, BK = 32, NO = BK / 8;
  constexpr int AP1 = NO * BM + 1;  // plane size: the tile + one all-zero slot that padded taps read instead of their row
  constexpr int SMEM_U4 = 2 * AP1 + 2 * NO * BN;
  __shared__ __attribute__((aligned(16))) uint4 smem[SMEM_U4];
  uint4* Ahi = smem;
  uint4* Alo = Ahi + AP1;
  uint4* Bhi = Alo + AP1;
  uint4* Blo = Bhi + NO * BN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lbs = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int split = lbs % splits, lb = lbs / splits;
  const int tile_n = lb % p.n_tiles_n, tile_m = lb / p.n_tiles_n;
  const int m0 = p.m_off + tile_m * (BM - 2) - 1, n0 = tile_n * BN;  // tile row j <-> output row m0 + j; rows 0 and BM - 1 are halo only
  const int oct = tid & 3, r0 = tid >> 2;
  const int il = lane & 31, h = lane >> 5;
  const int n_chunks = p.Cred / BK;
  const int all_groups = p.kh * n_chunks;  // one group = the three taps of (ty, chunk)
  const int g_begin = (int)((long long)all_groups * split / splits);
  int g_end = (int)((long long)all_groups * (split + 1) / splits);
  if (g_flags) {
    // row-block skip (pp_conv_opts.skip_flags): when none of the 32-row blocks of the gathered tensor that this tile can
    // reach (its rows +- one image row +- one pixel; skip_halo = widest level + 1) holds a non-zero, the sum is exactly
    // zero: no k-loop, the epilogue still writes bias / addend / mask.  Workgroup-uniform.
    int lo = m0 - skip_halo, hi = m0 + BM - 1 + skip_halo;
    lo = lo < 0 ? 0 : lo;
    hi = hi > p.M - 1 ? p.M - 1 : hi;
    int any = 0;
    for (int b = lo >> 5; b <= (hi >> 5); ++b) any |= g_flags[b];
    g_end = any ? g_end : g_begin;
  }

  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g_a), 0, a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_a1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(AP ? g_a1 : g_a), 0, AP ? a_bytes - 16 : a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_wh = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g_whi), 0, w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_wl = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g_wlo), 0, w_bytes, 0x00020000);

  // staged rows r0 + 64 * i: byte offset of the dx = 0 source pixel at ty = 0, row pitch (low 4 bits: source row y + dy exists, per ty)
  int s_base[TM], s_pitch[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int q = m0 + r0 + 64 * i;
    const RowPos r = decode_row(p, q < 0 ? 0 : q);
    const bool ok = q >= 0 && r.ok;
    const int x = r.xbase - p.off_x;  // dx = 0 <=> the output cell's own column
    s_base[i] = ((r.rowbase + r.ybase * r.SW + x) * p.ld_src + 8 * oct) * ES;
    int v = 0;
    for (int ty = 0; ty < p.kh; ++ty)
      if (ok && (unsigned)(r.ybase + ty * p.tsign) < (unsigned)r.SH) v |= 1 << ty;
    s_pitch[i] = (p.tsign * r.SW * p.ld_src * ES) | v;  // ld_src % 4 == 0 -> the pitch is a multiple of 16
  }
  // fragment rows of this lane: wm * 32 * TM + a * 32 + il -> validity bit per tap (9 bits each, two rows per register)
  unsigned f_valid[(TM + 1) / 2];
#pragma unroll
  for (int a = 0; a < (TM + 1) / 2; ++a) f_valid[a] = 0;
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const int q = m0 + wm * 32 * TM + a * 32 + il;
    const RowPos r = decode_row(p, q < 0 ? 0 : q);
    unsigned v = 0;
    int t = 0;
    for (int ty = 0; ty < p.kh; ++ty)
      for (int tx = 0; tx < 3; ++tx, ++t) {
        const int sy = r.ybase + ty * p.tsign, sx = r.xbase + tx * p.tsign;
        if (q >= 0 && r.ok && (unsigned)sy < (unsigned)r.SH && (unsigned)sx < (unsigned)r.SW) v |= 1u << t;
      }
    f_valid[a >> 1] |= v << (16 * (a & 1));
  }
  int b_base[TN];
#pragma unroll
  for (int i = 0; i < TN; ++i) {
    const int n = n0 + r0 + 64 * i;
    b_base[i] = n < w_rows ? (n * w_ld8 + oct) * 16 : PP_BUF_OOB;
  }
  const int b_tap = w_rows * w_ld8 * 16;

  float4 ra[TM][2];
  uint4 rah[TM], ral[TM];
  uint4 rbh[TN], rbl[TN];
  // group g <-> (chunk, ty).  Default (p.x_ty_inner, PP_CONV3_X_ORDER=1): kernel row innermost -- the three row-shifted tiles of
  // one channel chunk are fetched back to back (they overlap by all but one image row, so the second and third come from
  // L1 / L2 while they are hot): same time, FETCH_SIZE -10 % on the 512-wide head conv and -40 % on the 256-wide one
  // (profiles/r02_traffic.json).  PP_CONV3_X_ORDER=0: channel chunk innermost (round 1).
  const bool ty_inner = p.x_ty_inner != 0;
  int ty = ty_inner ? g_begin % p.kh : g_begin / n_chunks;
  int chunk = ty_inner ? g_begin / p.kh : g_begin - ty * n_chunks;  // group being LOADED

  auto load_a = [&]() {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      int vo = s_base[i] + __mul24(ty, s_pitch[i] & ~15) + chunk * (BK * ES);
      vo = ((s_pitch[i] >> ty) & 1) ? vo : PP_BUF_OOB;
      if (AP) {
        rah[i] = buf_load16(rs_a, vo, 0);
        ral[i] = buf_load16(rs_a1, vo, 0);
      } else {
        const uint4 q0 = buf_load16(rs_a, vo, 0), q1 = buf_load16(rs_a, vo + 16, 0);
        ra[i][0] = *reinterpret_cast<const float4*>(&q0);
        ra[i][1] = *reinterpret_cast<const float4*>(&q1);
      }
    }
  };
  auto load_b = [&](int tx) {
    const int b_uni = ((p.w_ty0 + ty) * p.w_kw + tx) * b_tap + chunk * (BK / 8 * 16);
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      rbh[i] = buf_load16(rs_wh, b_base[i], b_uni);
      rbl[i] = buf_load16(rs_wl, b_base[i], b_uni);
    }
  };
  auto split_a = [&]() {
    if (!AP) {
#pragma unroll
      for (int i = 0; i < TM; ++i) split8(ra[i][0], ra[i][1], &rah[i], &ral[i]);
    }
  };
  auto store_a = [&]() {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int slot = oct * BM + ((r0 + 64 * i + 2 * oct) & (BM - 1));
      Ahi[slot] = rah[i];
      Alo[slot] = ral[i];
    }
  };
  // CAP: (ty, chunk) is the group whose converted rows the registers hold; plane byte offset = f32 byte offset / 2
  const int ty_c = -p.off_y * p.tsign;  // kernel row with dy = 0
  auto capture = [&]() {
    if constexpr (CAP) {
      const __amdgpu_buffer_rsrc_t rs_ch = __builtin_amdgcn_make_buffer_rsrc(g_chi, 0, a_bytes, 0x00020000);
      const __amdgpu_buffer_rsrc_t rs_cl = __builtin_amdgcn_make_buffer_rsrc(g_clo, 0, a_bytes - 16, 0x00020000);
      if (ty == ty_c && chunk % p.n_tiles_n == tile_n) {  // uniform: the output-channel tiles of a row tile take turns
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int row = r0 + 64 * i;
          const int vo = s_base[i] + __mul24(ty, s_pitch[i] & ~15) + chunk * (BK * 4);
          const bool ok = ((s_pitch[i] >> ty) & 1) && row >= 1 && row <= BM - 2;
          const int co = ok ? vo : PP_BUF_OOB;  // packed planes: the f32 byte offset of the group
          buf_store16(rs_ch, rah[i], co);
          buf_store16(rs_cl, ral[i], co);
        }
      }
    }
  };
  auto store_b = [&]() {
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      const int slot = oct * BN + ((r0 + 64 * i + 2 * oct) & (BN - 1));
      Bhi[slot] = rbh[i];
      Blo[slot] = rbl[i];
    }
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // multiply the tile in LDS as tap (c_ty, TX): fragments of the gathered operand at row offset dx, zeroed where the tap pads
  auto mma_tile = [&](int c_ty, auto tx_c) {
    constexpr int TX = decltype(tx_c)::value;
    const int dx = p.off_x + TX * p.tsign;
    const unsigned tap_bits = (1u << (c_ty * 3 + TX)) * 0x10001u;  // the tap's bit in both 16-bit halves
    unsigned okm[(TM + 1) / 2];
#pragma unroll
    for (int a = 0; a < (TM + 1) / 2; ++a) okm[a] = f_valid[a] & tap_bits;
    unsigned a_ok = 0;
#pragma unroll
    for (int a = 0; a < TM; ++a) a_ok |= (((okm[a >> 1] >> (16 * (a & 1))) & 0xffffu) != 0 ? 1u : 0u) << a;
    // padded taps read the all-zero slot: one address select per fragment
    mma_step<TM, TN, BM, BN, 1>(acc, Ahi, Alo, Bhi, Blo, wm * 32 * TM + il + dx, wn * 32 * TN + il, h, a_ok, NO * BM);
  };

  std::integral_constant<int, 0> t0;
  std::integral_constant<int, 1> t1;
  std::integral_constant<int, 2> t2;
  if (threadIdx.x == 0) {
    Ahi[NO * BM] = make_uint4(0u, 0u, 0u, 0u);
    Alo[NO * BM] = make_uint4(0u, 0u, 0u, 0u);
  }
  load_a();
  load_b(0);
  split_a();
  store_a();
  store_b();
  __syncthreads();
  for (int g = g_begin; g < g_end; ++g) {
    const int c_ty = ty;
    // (CAP) the converted rows of this group are still in registers: their stores go out ahead of the tap's loads and
    // complete under its MFMAs (one vmcnt for loads and stores: issued later they would stall the next weight tile)
    capture();
    // tx = 0: the weight tile of tx = 1 is fetched under it
    load_b(1);
    __builtin_amdgcn_sched_barrier(0);
    mma_tile(c_ty, t0);
    __syncthreads();
    store_b();
    __syncthreads();
    // tx = 1
    load_b(2);
    __builtin_amdgcn_sched_barrier(0);
    mma_tile(c_ty, t1);
    __syncthreads();
    store_b();
    __syncthreads();
    // tx = 2: the next group's gathered rows and its first weight tile are fetched, converted and written
    {
      const bool more = g + 1 < g_end;  // past the end: rewind to group 0 (a harmless re-load)
      if (ty_inner) {
        ty += 1;
        const bool wt = ty == p.kh;
        ty = wt ? 0 : ty;
        chunk += wt ? 1 : 0;
      } else {
        chunk += 1;
        const bool wc = chunk == n_chunks;
        chunk = wc ? 0 : chunk;
        ty += wc ? 1 : 0;
      }
      chunk = more ? chunk : 0;
      ty = more ? ty : 0;
    }
    load_b(0);
    load_a();
    __builtin_amdgcn_sched_barrier(0);
    mma_tile(c_ty, t2);
    split_a();
    __syncthreads();
    store_b();
    store_a();
    __syncthreads();
  }
  // rows 0 and BM - 1 of the tile are halo: clear their accumulators' way out by making them out of range
  if (splits > 1) {
    float* slice = g_ws + (long long)split * (p.M - p.m_off) * p.ld_out;
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 32 * TM + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const int m = m0 + row;
#pragma unroll
        for (int b = 0; b < TN; ++b) {
          const int co = n0 + wn * 32 * TN + b * 32 + il;
          if (row >= 1 && row <= BM - 2 && m < p.M && co < ((p.Nout + 3) & ~3)) slice[(long long)(m - p.m_off) * p.ld_out + co] = acc[a][b][r];
        }
      }
    return;
  }
  epilogue3<TM, TN, OP, 4, false, true>(p, acc, smem, m0, n0, tid, wm, wn, il, h, g_bias, g_addend, g_mask, g_out, g_ohi, g_olo);
}

// epilogue arithmetic of the pointwise finishing kernels: v (+ addend) (masked by the ReLU source) (ReLU) -> f32 and / or planes;
// mo = row of the addend / mask / output tensors, co = first of four columns
__device__ __forceinline__ void finish4(const IgemmParams& p, float4 v, long long mo, int co, bool with_addend, const float* __restrict__ g_addend,
                                        const float* __restrict__ g_mask, float* __restrict__ g_out, void* __restrict__ g_ohi,
                                        void* __restrict__ g_olo) {
  if (with_addend) {
    if (p.add_hi) {
      const float4 a = planes_ld4(p.add_hi, p.add_lo, (mo * p.ld_add + co) >> 2);
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    } else if (g_addend) {
      const float4 a = *reinterpret_cast<const float4*>(g_addend + mo * p.ld_add + co);
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    }
  }
  if (p.mask_hi || g_mask) {
    const float4 k = p.mask_hi ? hi_ld4(p.mask_hi, (mo * p.ld_mask + co) >> 2) : *reinterpret_cast<const float4*>(g_mask + mo * p.ld_mask + co);
    v.x = k.x > 0.f ? v.x : 0.f; v.y = k.y > 0.f ? v.y : 0.f; v.z = k.z > 0.f ? v.z : 0.f; v.w = k.w > 0.f ? v.w : 0.f;
  }
  if (p.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
  if (g_out) *reinterpret_cast<float4*>(g_out + mo * p.ld_out + co) = v;
  if (g_ohi) planes_st4(g_ohi, g_olo, (mo * p.ld_out + co) >> 2, v);
}

// parity class without taps (e.g. the odd cells of a 1x1 stride-2 conv): dx = mask?(addend or 0) at the class rows
__global__ void class_fill_kernel(const IgemmParams p, const float* __restrict__ g_addend, const float* __restrict__ g_mask,
                                  float* __restrict__ g_out, void* __restrict__ g_ohi, void* __restrict__ g_olo) {
  const int n4 = (p.Nout + 3) >> 2;
  const long long total = (long long)p.M * n4;
  const int hw = p.seg[0].OH * p.seg[0].OW;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int m = (int)(i / n4), co = 4 * (int)(i - (long long)m * n4);
    const int n = m / hw, rem = m - n * hw, yq = rem / p.seg[0].OW, xq = rem - yq * p.seg[0].OW;
    const long long mo = (long long)(n * p.sc_H + 2 * yq + p.sc_cy) * p.sc_W + 2 * xq + p.sc_cx;
    finish4(p, make_float4(0.f, 0.f, 0.f, 0.f), mo, co, true, g_addend, g_mask, g_out, g_ohi, g_olo);
  }
}

// out = relu?(mask?(sum_s ws[s] + bias + addend)) over [M][ceil4(Nout)]
__global__ void splitk_finish_kernel(const IgemmParams p, int splits, const float* __restrict__ ws, const float* __restrict__ g_bias,
                                     const float* __restrict__ g_addend, const float* __restrict__ g_mask, float* __restrict__ g_out,
                                     void* __restrict__ g_ohi, void* __restrict__ g_olo) {
  const int n4 = (p.Nout + 3) >> 2;
  const int rows = p.M - p.m_off;  // (m_off: the launch covers the rows from there on)
  const long long total = (long long)rows * n4, slice = (long long)rows * p.ld_out;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int mr = (int)(i / n4), co = 4 * (int)(i - (long long)mr * n4);
    const int m = p.m_off + mr;
    const float* w = ws + (long long)mr * p.ld_out + co;
    float4 v = *reinterpret_cast<const float4*>(w);
    for (int s = 1; s < splits; ++s) {
      const float4 q = *reinterpret_cast<const float4*>(w + s * slice);
      v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    }
    if (g_bias) { const float4 b = *reinterpret_cast<const float4*>(g_bias + co); v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w; }
    finish4(p, v, (long long)m, co, true, g_addend, g_mask, g_out, g_ohi, g_olo);
  }
}

// split-K of the row-list launch: block j of the list <-> compact slice rows 32 j .. 32 j + 31
__global__ void rl_splitk_finish_kernel(const IgemmParams p, int splits, const float* __restrict__ ws, const int* __restrict__ g_rl,
                                        const float* __restrict__ g_bias, const float* __restrict__ g_addend, const float* __restrict__ g_mask,
                                        float* __restrict__ g_out, void* __restrict__ g_ohi, void* __restrict__ g_olo) {
  const int j = blockIdx.x;
  if (j >= g_rl[0]) return;
  const int n4 = (p.Nout + 3) >> 2;
  const long long slice = (((long long)p.M + 31) & ~31ll) * p.ld_out;
  const int m0 = g_rl[1 + j] * 32, nr = min(32, p.M - m0);
  for (int i = threadIdx.x; i < nr * n4; i += blockDim.x) {
    const int r = i / n4, co = 4 * (i - r * n4);
    const float* w = ws + ((long long)j * 32 + r) * p.ld_out + co;
    float4 v = *reinterpret_cast<const float4*>(w);
    for (int s = 1; s < splits; ++s) {
      const float4 q = *reinterpret_cast<const float4*>(w + s * slice);
      v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    }
    if (g_bias) { const float4 b = *reinterpret_cast<const float4*>(g_bias + co); v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w; }
    finish4(p, v, (long long)(m0 + r), co, true, g_addend, g_mask, g_out, g_ohi, g_olo);
  }
}

// ---- sparse data gradient of a 3x3 stride-1 conv: which 32-row OUTPUT blocks can a non-zero of dy reach? ----
// Output row m reads dy rows m + dy * W + dx, dy, dx in {-1, 0, 1} (W = width of m's level): block b is live when a flagged
// dy block intersects one of the three 34-row windows [32 b - 1 + j W, 32 b + 32 + j W], j = -1, 0, 1 -- exact in 2-D up to
// the 32-cell granularity (image / level boundaries are ignored: conservative).
__global__ void rl_dilate_kernel(const IgemmParams p, const unsigned char* __restrict__ in_flags, unsigned char* __restrict__ out_flags,
                                 int n_blocks) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_blocks) return;
  const int r_lo = 32 * b, r_hi = min(32 * b + 31, p.M - 1);
  int any = 0;
  for (int s = 0; s < p.n_seg; ++s) {
    const int seg_lo = p.seg[s].row_begin, seg_hi = (s + 1 < p.n_seg ? p.seg[s + 1].row_begin : p.M) - 1;
    if (r_hi < seg_lo || r_lo > seg_hi) continue;
    const int W = p.seg[s].OW;
    for (int j = -1; j <= 1; ++j) {
      int lo = r_lo - 1 + j * W, hi = r_hi + 1 + j * W;
      lo = lo < 0 ? 0 : lo;
      hi = hi > p.M - 1 ? p.M - 1 : hi;
      for (int q = lo >> 5; q <= (hi >> 5); ++q) any |= in_flags[q];
    }
  }
  out_flags[b] = any ? 1 : 0;
}

// rows of the blocks that no non-zero reaches: dx = mask?(addend or 0)
__global__ void rl_fill_kernel(const IgemmParams p, const unsigned char* __restrict__ live, const float* __restrict__ g_addend,
                               const float* __restrict__ g_mask, float* __restrict__ g_out, void* __restrict__ g_ohi, void* __restrict__ g_olo) {
  const int b = blockIdx.x;
  if (live[b]) return;
  const int n4 = (p.Nout + 3) >> 2;
  const int r0 = 32 * b, nr = min(32, p.M - r0);
  if (g_ohi && !g_out && !g_addend && p.Nout == p.ld_out && (p.ld_out & 7) == 0 && (p.add_hi == nullptr || (p.ld_add & 7) == 0) &&
      (p.mask_hi == nullptr || (p.ld_mask & 7) == 0)) {
    // planes in and out, whole rows: the block is nr * ld_out / 8 contiguous 32-byte groups -> 16-byte accesses throughout
    // (the 8-byte form below ran at half the store rate: 46 us per launch in the step)
    const int n8 = nr * (p.ld_out >> 3);
    uint4* dst = reinterpret_cast<uint4*>(g_ohi) + 2 * (long long)r0 * (p.ld_out >> 3);
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
    for (int i = threadIdx.x; i < n8; i += blockDim.x) {
      uint4 oh = z4, ol = z4;
      if (p.add_hi) {
        const int r = i / (p.ld_out >> 3), g8 = i - r * (p.ld_out >> 3);
        const uint4* a = reinterpret_cast<const uint4*>(p.add_hi) + 2 * ((long long)(r0 + r) * (p.ld_add >> 3) + g8);
        oh = a[0];
        ol = a[1];
        if (p.mask_hi) {  // keep the addend where the ReLU source is positive (hi > 0: sign bit clear and not zero)
          const uint4 k = reinterpret_cast<const uint4*>(p.mask_hi)[2 * ((long long)(r0 + r) * (p.ld_mask >> 3) + g8)];
          const unsigned kk[4] = {k.x, k.y, k.z, k.w};
          unsigned hh[4] = {oh.x, oh.y, oh.z, oh.w}, ll[4] = {ol.x, ol.y, ol.z, ol.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const unsigned lo_ok = ((kk[j] & 0x8000u) == 0u && (kk[j] & 0x7fffu) != 0u) ? 0x0000ffffu : 0u;
            const unsigned hi_ok = ((kk[j] & 0x80000000u) == 0u && (kk[j] & 0x7fff0000u) != 0u) ? 0xffff0000u : 0u;
            hh[j] &= (lo_ok | hi_ok);
            ll[j] &= (lo_ok | hi_ok);
          }
          oh = make_uint4(hh[0], hh[1], hh[2], hh[3]);
          ol = make_uint4(ll[0], ll[1], ll[2], ll[3]);
        }
      }
      dst[2 * i] = oh;
      dst[2 * i + 1] = ol;
    }
    return;
  }
  for (int i = threadIdx.x; i < nr * n4; i += blockDim.x) {
    const int r = i / n4, co = 4 * (i - r * n4);
    const long long m = r0 + r;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    if (g_addend || p.add_hi) {
      finish4(p, z, m, co, true, g_addend, g_mask, g_out, g_ohi, g_olo);
    } else {  // (without an addend the row is zero whatever the mask says: nothing to read)
      if (g_out) *reinterpret_cast<float4*>(g_out + m * p.ld_out + co) = z;
      if (g_ohi) {
        reinterpret_cast<uint2*>(g_ohi)[pk4((m * p.ld_out + co) >> 2)] = make_uint2(0u, 0u);
        reinterpret_cast<uint2*>(g_olo)[pk4((m * p.ld_out + co) >> 2)] = make_uint2(0u, 0u);
      }
    }
  }
}

// adds the split-K slices of rows p.m_off .. M - 1 and writes the output (planes included)
static void launch_splitk_finish(hipStream_t st, const IgemmParams& p, int splits, const float* ws, unsigned blocks, void* ohi, void* olo) {
  hipLaunchKernelGGL(splitk_finish_kernel, dim3(blocks), dim3(256), 0, st, p, splits, ws, p.bias, p.addend, p.mask_src, p.out, ohi, olo);
}

// the launch of igemm3f_kernel.  AP / OP: the gathered operand / the output (ohi, olo) as planes; SC: one parity class of a stride-2
// data gradient; RL: over the listed blocks (list, srcflags).  splits > 1: partial sums to ws, the caller runs the finish
template <int TM, int TN, bool AP, bool OP, bool SC, bool RL>
static void launch_igemm3f(hipStream_t st, unsigned grid, const IgemmParams& p, const Igemm3Args& a, void* ohi, void* olo, int splits, float* ws,
                           const int* list, const unsigned char* srcflags) {
  const unsigned a_bytes = (unsigned)(p.src_rows * (long long)p.ld_src * 4), w_bytes = (unsigned)((long long)p.w_taps * a.w_rows * a.w_ld8 * 16);
  hipLaunchKernelGGL((igemm3f_kernel<TM, TN, AP, OP, SC, RL>), dim3(grid), dim3(256), 0, st, p, AP ? a.ahi : (const void*)p.src, AP ? a.alo : nullptr,
                     a_bytes, a.whi, a.wlo, w_bytes, p.bias, p.addend, p.mask_src, p.out, (uint2*)(OP ? ohi : nullptr), (uint2*)(OP ? olo : nullptr),
                     a.w_rows, a.w_ld8, splits, ws, list, srcflags);
}

// the whole sparse bwd-data: dilate -> compact -> igemm3f over the listed blocks -> fill the others.  scratch: n_blocks bytes
// + (n_blocks + 1) ints behind the caller's flags / list (pp_row_block_list documents the sizes).
// dy_flags == NULL (forward, pp_conv_opts.out_flags): out_flags are given -- no dilation, and the rows of the other blocks
// are left as they are (fill = false).
template <int TM, int TN>
static void launch_igemm3_rowlist(hipStream_t st, IgemmParams& p, const Igemm3Args& a, const PpIgemmPlan& pl, const unsigned char* dy_flags,
                                  unsigned char* out_flags, int* out_list, bool fill) {
  // (dy_flags also masks the gather: rows of the gathered tensor outside its flagged blocks are never fetched)
  const int nb = (p.M + 31) / 32, splits = pl.splits;
  float* const ws = splits > 1 ? a.ws : nullptr;
  const dim3 wg(256);
  p.n_tiles_n = pl.n_tiles_n;
  if (dy_flags) hipLaunchKernelGGL(rl_dilate_kernel, dim3((unsigned)((nb + 255) / 256)), wg, 0, st, p, dy_flags, out_flags, nb);
  PP_API(pp3_launch_row_block_compact)(st, out_flags, nb, out_list);
  if (a.ahi && !a.ohi)  // planes in, float32 out (a head's last conv in the forward pass)
    launch_igemm3f<TM, TN, true, false, false, true>(st, pl.grid, p, a, nullptr, nullptr, splits, ws, out_list, dy_flags);
  else if (a.ahi)  // planes in, planes out
    launch_igemm3f<TM, TN, true, true, false, true>(st, pl.grid, p, a, a.ohi, a.olo, splits, ws, out_list, dy_flags);
  else
    launch_igemm3f<TM, TN, false, false, false, true>(st, pl.grid, p, a, nullptr, nullptr, splits, ws, out_list, dy_flags);
  if (pl.finish_blocks)
    hipLaunchKernelGGL(rl_splitk_finish_kernel, dim3(pl.finish_blocks), wg, 0, st, p, splits, (const float*)a.ws, (const int*)out_list, p.bias,
                       p.addend, p.mask_src, p.out, a.ohi, a.olo);
  // In place on the addend (dx == the running sum of the other data gradients of this tensor, no ReLU mask): the rows that no
  // non-zero reaches already hold their value -- nothing to fill (the shared pyramid features' gradient: 103 MB not moved).
  const bool in_place = (a.ohi != nullptr && p.add_hi == (const void*)a.ohi && p.ld_add == p.ld_out && !p.out && !p.addend && !p.mask_hi &&
                         !p.mask_src && !p.relu) ||
                        (p.out != nullptr && p.addend == p.out && p.ld_add == p.ld_out && !a.ohi && !p.add_hi && !p.mask_hi && !p.mask_src && !p.relu);
  if (fill && !in_place)
    hipLaunchKernelGGL(rl_fill_kernel, dim3((unsigned)nb), wg, 0, st, p, (const unsigned char*)out_flags, p.addend, p.mask_src, p.out, a.ohi, a.olo);
}

// the launches of one plan (conv_plan.h: pp_plan_igemm decided everything) on its tile
template <int TM, int TN>
static void launch_igemm3(hipStream_t st, IgemmParams& p, const Igemm3Args& a, const PpIgemmPlan& pl) {
  const dim3 wg(256);
  const unsigned a_bytes = (unsigned)(p.src_rows * (long long)p.ld_src * 4), w_bytes = (unsigned)((long long)p.w_taps * a.w_rows * a.w_ld8 * 16);
  const int splits = pl.splits;
  float* const ws = splits > 1 ? a.ws : nullptr;  // partial sums -> scratch; splitk_finish_kernel writes the output
  uint2 *const no_hi = nullptr, *const no_lo = nullptr;
  const std::true_type yes{};
  const std::false_type no{};
  p.n_tiles_n = pl.n_tiles_n;
  p.x_ty_inner = pl.x_ty_inner;
  if (pl.capture_first) PP_API(pp3_split_capture_pass)(st, p, a.chi, a.clo);
  // igemm3x on the rows of q from q.m_off on.  CAP: the split of the gathered f32 operand is captured; AP / OP: gathered operand /
  // output as planes (the 256-row tile has the plane-stored forms only: conv_plan.h)
  auto go_x = [&](auto cap, auto ap, auto op, const IgemmParams& q, unsigned grid, int q_splits, float* q_ws, const unsigned char* flags) {
    constexpr bool CAP = decltype(cap)::value, AP = decltype(ap)::value, OP = decltype(op)::value;
    if constexpr (AP || TM <= 2)
      hipLaunchKernelGGL((igemm3x_kernel<TM, TN, CAP, AP, OP>), dim3(grid), wg, 0, st, q, AP ? a.ahi : (const void*)q.src, AP ? a.alo : nullptr, a_bytes,
                         a.whi, a.wlo, w_bytes, q.bias, q.addend, q.mask_src, q.out, OP ? (uint2*)a.ohi : no_hi, OP ? (uint2*)a.olo : no_lo, a.w_rows,
                         a.w_ld8, q_splits, q_ws, CAP ? a.chi : nullptr, CAP ? a.clo : nullptr, flags, pl.skip_halo);
  };
  switch (pl.family) {
    case PP_IGEMM3F_CLASS:
      if (a.ahi) launch_igemm3f<TM, TN, true, true, true, false>(st, pl.grid, p, a, a.ohi, a.olo, 1, nullptr, nullptr, nullptr);
      else launch_igemm3f<TM, TN, false, false, true, false>(st, pl.grid, p, a, nullptr, nullptr, 1, nullptr, nullptr, nullptr);
      return;
    case PP_IGEMM4X:
      if constexpr (TM == 2 && TN == 2) {
        PP_API(pp3_launch_igemm4x)(st, p, a, pl);
        if (pl.tail_splits > 1) {  // the rows of the last, partly filled round
          IgemmParams q = p;
          q.m_off = pl.tail_m_off;
          go_x(no, yes, no, q, pl.tail_grid, pl.tail_splits, a.ws, nullptr);
          launch_splitk_finish(st, q, pl.tail_splits, a.ws, pl.finish_blocks, a.ohi, a.olo);
        }
      }
      return;
    case PP_IGEMM4X2:
      if constexpr (TM == 2 && TN == 2) PP_API(pp3_launch_igemm4x)(st, p, a, pl);
      return;
    case PP_IGEMM4P:
      if constexpr (TM == 2 && TN == 2)
        PP_API(pp4_launch_igemm4p)(st, p, a.ahi, a.whi, a.wlo, a.w_rows, a.w_ld8, a.ohi, a.olo, splits, ws, pl.grid, pl.stages);
      break;
    case PP_IGEMM3X_CAPTURE: go_x(yes, no, no, p, pl.grid, splits, ws, a.flags); break;
    case PP_IGEMM3X_PP: go_x(no, yes, yes, p, pl.grid, splits, ws, a.flags); break;
    case PP_IGEMM3X_PF: go_x(no, yes, no, p, pl.grid, splits, ws, a.flags); break;
    case PP_IGEMM3X_FP: go_x(no, no, yes, p, pl.grid, splits, ws, a.flags); break;
    case PP_IGEMM3X_FF: go_x(no, no, no, p, pl.grid, splits, ws, a.flags); break;
    default: {  // PP_IGEMM3F / PP_IGEMM3, four operand forms each
      void *const ohi = splits > 1 ? nullptr : a.ohi, *const olo = splits > 1 ? nullptr : a.olo;
      auto go = [&](auto ap, auto op) {
        constexpr bool AP = decltype(ap)::value, OP = decltype(op)::value;
        if (pl.family == PP_IGEMM3F)
          launch_igemm3f<TM, TN, AP, OP, false, false>(st, pl.grid, p, a, ohi, olo, splits, ws, nullptr, nullptr);
        else
          hipLaunchKernelGGL((igemm3_kernel<TM, TN, AP, OP>), dim3(pl.grid), wg, 0, st, p, p.src, (const uint4*)(AP ? a.ahi : nullptr),
                             (const uint4*)(AP ? a.alo : nullptr), (const uint4*)a.whi, (const uint4*)a.wlo, p.bias, p.addend, p.mask_src, p.out,
                             (uint2*)ohi, (uint2*)olo, a.w_rows, a.w_ld8);
      };
      if (a.ahi && ohi) go(yes, yes);
      else if (a.ahi) go(yes, no);
      else if (ohi) go(no, yes);
      else go(no, no);
    }
  }
  if (pl.finish_blocks) launch_splitk_finish(st, p, splits, a.ws, pl.finish_blocks, a.ohi, a.olo);
}

// the merged stride-2 data gradient: one launch on the route's tile (p: the shared fields of its classes)
template <int TM, int TN>
static void launch_igemm3m(hipStream_t st, IgemmParams& p, const Igemm3Args& a, const DgradS2Route& r) {
  const dim3 grid(r.g.grid), wg(256);
  const unsigned a_bytes = (unsigned)(p.src_rows * (long long)p.ld_src * 4), w_bytes = (unsigned)((long long)p.w_taps * a.w_rows * a.w_ld8 * 16);
  p.n_tiles_n = r.pl.n_tiles_n;
  auto go = [&](auto planes) {  // operands all planes or all float32
    constexpr bool P = decltype(planes)::value;
    hipLaunchKernelGGL((igemm3m_kernel<TM, TN, P, P>), grid, wg, 0, st, p, r.g, P ? a.ahi : (const void*)p.src, P ? a.alo : nullptr, a_bytes, a.whi, a.wlo,
                       w_bytes, p.addend, p.mask_src, p.out, (uint2*)(P ? a.ohi : nullptr), (uint2*)(P ? a.olo : nullptr), a.w_rows, a.w_ld8);
  };
  if (a.ahi) go(std::true_type{});
  else go(std::false_type{});
}

}  // namespace

void PP_API(pp3_launch_igemm)(hipStream_t st, IgemmParams& p, const Igemm3Args& a, const PpIgemmPlan& pl) {
  if (pl.tm == 4) launch_igemm3<4, 2>(st, p, a, pl);
  else if (pl.tm == 2 && pl.tn == 2) launch_igemm3<2, 2>(st, p, a, pl);
  else if (pl.tm == 1 && pl.tn == 2) launch_igemm3<1, 2>(st, p, a, pl);
  else if (pl.tm == 2 && pl.tn == 1) launch_igemm3<2, 1>(st, p, a, pl);
  else launch_igemm3<1, 1>(st, p, a, pl);
}

void PP_API(pp3_launch_igemm_s2)(hipStream_t st, IgemmParams& p, const Igemm3Args& a, const DgradS2Route& r) {
  if (r.pl.tm == 4) launch_igemm3m<4, 2>(st, p, a, r);
  else if (r.pl.tm == 2 && r.pl.tn == 2) launch_igemm3m<2, 2>(st, p, a, r);
  else if (r.pl.tm == 1 && r.pl.tn == 2) launch_igemm3m<1, 2>(st, p, a, r);
  else if (r.pl.tm == 2 && r.pl.tn == 1) launch_igemm3m<2, 1>(st, p, a, r);
  else launch_igemm3m<1, 1>(st, p, a, r);
}

// (pl.tm: 2 = 128 x 128 tiles, 1 = 64 x 128)
void PP_API(pp3_launch_igemm_rowlist)(hipStream_t st, IgemmParams& p, const Igemm3Args& a, const PpIgemmPlan& pl, const unsigned char* dy_flags,
                                      unsigned char* out_flags, int* out_list, bool fill) {
  if (pl.tm == 2) launch_igemm3_rowlist<2, 2>(st, p, a, pl, dy_flags, out_flags, out_list, fill);
  else launch_igemm3_rowlist<1, 2>(st, p, a, pl, dy_flags, out_flags, out_list, fill);
}

void PP_API(pp3_launch_class_fill)(hipStream_t st, const IgemmParams& p, unsigned blocks, const float* addend, const float* mask, float* out, void* ohi,
                                   void* olo) {
  hipLaunchKernelGGL(class_fill_kernel, dim3(blocks), dim3(256), 0, st, p, addend, mask, out, ohi, olo);
}

void PP_API(pp3_launch_rl_dilate)(hipStream_t st, const IgemmParams& p, const unsigned char* in_flags, unsigned char* out_flags, int n_blocks) {
  hipLaunchKernelGGL(rl_dilate_kernel, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, st, p, in_flags, out_flags, n_blocks);
}
