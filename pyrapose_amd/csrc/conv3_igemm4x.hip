// igemm4x: the LDS-DMA form of the 3x3 stride-1 convolution on plane-stored operands, and its launcher (conv3.h).  The arithmetic
// of the family is described at the head of conv3.hip.
#include "conv3_unit.h"
#include "conv3.h"

namespace {

// ---- igemm4x: igemm3x's arithmetic and tap-row reuse on a multi-stage LDS-DMA pipeline (PP_CONV3_DMA=0 turns it off) ----
// Why: the 128 x 128, two-barriers-per-tap loop of igemm3x prefetches one tap ahead through registers; with an L2 hit rate of 90 % a
// wave's four weight loads per tap contain a miss every third tap, and three waves per SIMD cannot cover it (46-59 % of the wave
// cycles in s_waitcnt, MFMA pipe 48 % busy).  Here: ONE workgroup of 8 waves per CU, tile 256 x 128 (wave tile 64 x 64 as
// before), both operands reach LDS by buffer_load ... lds (no staging registers) into rings -- 2 stages of the gathered tile (one
// per (ty, chunk) group, loaded a group = three taps ahead), 3 stages of the weight tile (the stage of a tap is its tx; loaded two
// taps ahead) -- that stay in flight ACROSS the one barrier per tap; the waits are counted (vmcnt 6 / 2 / 2), never 0 in the loop.
//  * A wave-instruction of LDS-DMA writes 64 lane-consecutive 16-byte slots, so the LDS image is shaped on the SOURCE side: the
//    lane at slot s fetches the piece that belongs at s.  Images (planes_fmt.h LAY 1): row-major, XOR-swizzled pieces -- one
//    instruction moves 8 rows x 128 contiguous bytes of the gathered operand ([hi0 lo0 .. hi3 lo3] of a row's 32-channel chunk:
//    full lines; fragment-shaped 16-byte pieces of 64 different lines per instruction cost 15 % of the kernel) or 16 rows x 64
//    bytes of a weight plane.  Padding rows are out-of-range offsets (the DMA writes zeros).
//  * Every stage is an LDS object of its own: the compiler tracks LDS-DMA per object (alias scopes), so the waits it inserts in
//    front of a fragment read are COUNTED and cover the DMA into that stage only (one shared array: vmcnt(0) before every read).
//  * One workgroup per CU makes a last, partly filled round cost a whole round: the host gives whole rounds to this kernel and
//    the remaining rows to igemm3x with the reduction split over a round's worth of workgroups (IgemmParams::m_off).
// Same products in the same order as igemm3x: the rows of the whole rounds are bit-identical to it.  Planes in, planes out,
// 3x3 stride 1, kernel row innermost (x_ty_inner), w_rows % 128 == 0, at least two rounds of tiles (PP_CONV3_DMA_MIN).
// Measured (P16, same box): 422-434 us against 499 on a tail-free 512-channel shape (1.16x), the regression-head launch 486 against
// 577 us (1.19x, 490 TFLOP/s); bf16 pairs 1.04x; training step +3.1 %.
// NWM = 4: the form above (8 waves, 256 x 128, one workgroup per CU, weight ring of three stages = 112 KB of LDS).
// NWM = 2 (round 4): 4 waves, 128 x 128, TWO workgroups per CU -- gathered ring of 2 x 16 KB + weight ring of 2 x 16 KB = 64 KB
// each -- for the launches that cannot fill two rounds of 256-row tiles (the 256-channel heads, the FPN 3x3): the weight tile is
// fetched ONE tap ahead (into the stage the previous tap has just left), the gathered tile two taps ahead; the second workgroup
// of the CU covers the waits.  Same products in the same order as igemm3x either way.
template <bool OP, int VAR = 0, int NWM = 4>
__global__ __launch_bounds__(128 * NWM, NWM == 4 ? 1 : 2) void igemm4x_kernel(
    const IgemmParams p, const void* __restrict__ g_a, const void* __restrict__ g_a1, unsigned a_bytes, const void* __restrict__ g_whi,
    const void* __restrict__ g_wlo, unsigned w_bytes, const float* __restrict__ g_bias, const float* __restrict__ g_addend,
    const float* __restrict__ g_mask, float* __restrict__ g_out, uint2* __restrict__ g_ohi, uint2* __restrict__ g_olo, int w_rows, int w_ld8) {
  constexpr int TM = 2, TN = 2, NW = 2 * NWM, BM = 32 * TM * NWM, BN = 128, BK = 32, NO = BK / 8, ES = 4;
  constexpr int BST = NWM == 4 ? 3 : 2;  // stages of the weight ring
  constexpr int BI = 128 / (16 * NW);    // LDS-DMA instructions per wave and weight plane (16 rows x 64 bytes each)
  constexpr int A_STAGE = 8 * BM + 2, B_STAGE = 2 * NO * BN;  // (gathered: 8 pieces per row + the two zero slots; weights: hi + lo regions)
  // every stage is an LDS object of its own: the compiler's LDS-DMA tracking (alias scopes per object) then inserts COUNTED vmcnt
  // waits in front of a fragment read -- for the DMA into that stage only -- instead of draining everything in flight
  __shared__ __attribute__((aligned(16))) uint4 sA0[A_STAGE];
  __shared__ __attribute__((aligned(16))) uint4 sA1[A_STAGE];
  __shared__ __attribute__((aligned(16))) uint4 sB0[B_STAGE];
  __shared__ __attribute__((aligned(16))) uint4 sB1[B_STAGE];
  __shared__ __attribute__((aligned(16))) uint4 sB2[BST == 3 ? B_STAGE : 1];
  auto stA = [&](auto k) -> uint4* {
    if constexpr (decltype(k)::value == 0) return sA0; else return sA1;
  };
  auto stB = [&](auto k) -> uint4* {
    if constexpr (decltype(k)::value == 0) return sB0; else return sB1;
  };

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int lb = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int tile_n = lb % p.n_tiles_n, tile_m = lb / p.n_tiles_n;
  const int m0 = tile_m * (BM - 2) - 1, n0 = tile_n * BN;
  const int il = lane & 31, h = lane >> 5;
  const int n_chunks = p.Cred / BK;
  const int G = p.kh * n_chunks;  // groups: (chunk, ty), ty innermost

  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g_a), 0, a_bytes, 0x00020000);
  (void)g_a1;  // (packed planes: the lo halves are pieces of the same 128-byte chunks, reached through g_a)
  const __amdgpu_buffer_rsrc_t rs_wh = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g_whi), 0, w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_wl = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g_wlo), 0, w_bytes, 0x00020000);

  // DMA lanes (LDS images of planes_fmt.h LAY 1, filled in FULL lines).  Gathered tile: one instruction = 8 rows x 8 pieces (the
  // 128 contiguous bytes [hi0 lo0 .. hi3 lo3] of a row's 32-channel chunk); wave w owns rows 32 w .. 32 w + 31 in four instructions;
  // the lane at LDS piece position q of row r fetches piece q ^ ((r / 2) mod 8).  Weight tile, per plane: one instruction = 16
  // rows x 4 pieces (64 contiguous bytes); wave w owns rows 16 (BI w + i) .. + 15, i < BI; piece q of row n is octet q ^ ((n / 4) mod 4).
  int s_base[4], s_pitch[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int j = 32 * wave + 8 * c + (lane >> 3);
    const int piece = (lane & 7) ^ ((j >> 1) & 7);
    const int q = m0 + j;
    const RowPos r = decode_row(p, q < 0 ? 0 : q);
    const bool ok = q >= 0 && r.ok;
    const int x = r.xbase - p.off_x;
    s_base[c] = (r.rowbase + r.ybase * r.SW + x) * p.ld_src * ES + 16 * piece;
    int v = 0;
    for (int ty = 0; ty < 3; ++ty)
      if (ok && (unsigned)(r.ybase + ty * p.tsign) < (unsigned)r.SH) v |= 1 << ty;
    s_pitch[c] = (p.tsign * r.SW * p.ld_src * ES) | v;
  }
  int b_dma[BI];
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    const int b_row = 16 * (BI * wave + i) + (lane >> 2);
    const int b_n = n0 + b_row;
    b_dma[i] = b_n < w_rows ? (b_n * w_ld8 + ((lane & 3) ^ ((b_row >> 2) & 3))) * 16 : PP_BUF_OOB;
  }
  const int b_tap = w_rows * w_ld8 * 16;

  unsigned f_valid = 0;
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const int q = m0 + wm * 32 * TM + a * 32 + il;
    const RowPos r = decode_row(p, q < 0 ? 0 : q);
    unsigned v = 0;
    int t = 0;
    for (int ty = 0; ty < 3; ++ty)
      for (int tx = 0; tx < 3; ++tx, ++t) {
        const int sy = r.ybase + ty * p.tsign, sx = r.xbase + tx * p.tsign;
        if (q >= 0 && r.ok && (unsigned)sy < (unsigned)r.SH && (unsigned)sx < (unsigned)r.SW) v |= 1u << t;
      }
    f_valid |= v << (16 * (a & 1));
  }

  auto dma_a = [&](int g, uint4* st) {  // the gathered tile of group g -> stage st
    const int ty = g % 3, chunk = g / 3;
    uint4* const dst = st + 8 * 32 * wave;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      int vo = s_base[c] + __mul24(ty, s_pitch[c] & ~15) + chunk * (BK * ES);
      vo = ((s_pitch[c] >> ty) & 1) ? vo : PP_BUF_OOB;
      dma16(rs_a, dst + 64 * c, vo, 0);
    }
  };
  auto dma_b = [&](int g, int tx, uint4* st) {  // the weight tile of tap (group g, tx) -> stage st
    const int ty = g % 3, chunk = g / 3;
    const int b_uni = ((p.w_ty0 + ty) * p.w_kw + tx) * b_tap + chunk * (BK / 8 * 16);
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      uint4* const hi = st + 4 * 16 * (BI * wave + i);
      dma16(rs_wh, hi, b_dma[i], b_uni);
      dma16(rs_wl, hi + NO * BN, b_dma[i], b_uni);
    }
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  auto mma_tile = [&](int c_ty, int TX, const uint4* Ahi, const uint4* Bhi) {
    const int dx = p.off_x + TX * p.tsign;
    const unsigned tap_bits = (1u << (c_ty * 3 + TX)) * 0x10001u;
    const unsigned okm = f_valid & tap_bits;
    unsigned a_ok = 0;
#pragma unroll
    for (int a = 0; a < TM; ++a) a_ok |= (((okm >> (16 * (a & 1))) & 0xffffu) != 0 ? 1u : 0u) << a;
    if (VAR & 2) __builtin_amdgcn_s_setprio(1);
    mma_step<TM, TN, BM, BN, (VAR & 4) ? 2 : ((VAR & 1) ? 0 : 1), 1>(acc, Ahi, Ahi, Bhi, Bhi + NO * BN, wm * 32 * TM + il + dx, wn * 32 * TN + il, h, a_ok, 8 * BM);
    if (VAR & 2) __builtin_amdgcn_s_setprio(0);
  };
  std::integral_constant<int, 0> c0;
  std::integral_constant<int, 1> c1;
  auto tap_end = [&](auto n) {  // all but the n youngest DMAs of this wave have landed; then every wave's have
    constexpr int N = decltype(n)::value;
    if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else static_assert(N == 0, "tap_end: count");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  // BST == 3: weight ring of THREE stages: the stage of a tap is its tx (compile time without unrolling over groups), the tile of tap
  // t + 2 goes into the stage tap t - 1 has just left; gathered ring of two stages (unrolled over two groups), loaded one group ahead.
  // Issue order at a tap's start: [gathered tile of the next group, at tx == 0], weight tile of tap t + 2.  At the end of tap t the
  // tile of tap t + 1 (issued at tap t - 1) must have landed: instructions issued after it = tx 0: 4 (A) + 2 = 6; tx 1: 2;
  // tx 2: 2 -- and the gathered tile of group g + 1 (issued at tx 0, before the weight tile waited for at tx 1) is then in.
  // BST == 2: the stage of a tap is the parity of its index in a PAIR of groups (u = 3 K + tx); at a tap's start the weight tile of
  // tap t + 1 goes into the other stage (all waves have left it: the barrier that ended tap t - 1), then -- at tx == 0 -- the
  // gathered tile of the next group; at the tap's end the weight tile must be in: everything but the 4 gathered DMAs issued behind
  // it at tx 0 (they have until the end of tx 1), everything at tx 1 and tx 2.
  auto group = [&](int g, auto k) {
    constexpr int K = decltype(k)::value;
    const int c_ty = g % 3;
    const int gn = g + 1 < G ? g + 1 : 0;  // past the end: group 0 again (a harmless re-load)
    uint4* const Ahi = stA(std::integral_constant<int, K & 1>{});
    if constexpr (BST == 3) {
      dma_a(gn, stA(std::integral_constant<int, (K + 1) & 1>{}));
      dma_b(g, 2, sB2);
      mma_tile(c_ty, 0, Ahi, sB0);
      tap_end(std::integral_constant<int, 6>{});
      dma_b(gn, 0, sB0);
      mma_tile(c_ty, 1, Ahi, sB1);
      tap_end(std::integral_constant<int, 2>{});
      dma_b(gn, 1, sB1);
      mma_tile(c_ty, 2, Ahi, sB2);
      tap_end(std::integral_constant<int, 2>{});
    } else {
      constexpr int U = 3 * K;
      dma_b(g, 1, stB(std::integral_constant<int, (U + 1) & 1>{}));
      dma_a(gn, stA(std::integral_constant<int, (K + 1) & 1>{}));
      mma_tile(c_ty, 0, Ahi, stB(std::integral_constant<int, U & 1>{}));
      tap_end(std::integral_constant<int, 4>{});
      dma_b(g, 2, stB(std::integral_constant<int, U & 1>{}));
      mma_tile(c_ty, 1, Ahi, stB(std::integral_constant<int, (U + 1) & 1>{}));
      tap_end(std::integral_constant<int, 0>{});
      dma_b(gn, 0, stB(std::integral_constant<int, (U + 1) & 1>{}));
      mma_tile(c_ty, 2, Ahi, stB(std::integral_constant<int, U & 1>{}));
      tap_end(std::integral_constant<int, 0>{});
    }
  };

  if (tid == 0) {  // the two all-zero slots (hi, lo = slot ^ 1) behind each gathered stage
    sA0[8 * BM] = make_uint4(0u, 0u, 0u, 0u);
    sA0[8 * BM + 1] = make_uint4(0u, 0u, 0u, 0u);
    sA1[8 * BM] = make_uint4(0u, 0u, 0u, 0u);
    sA1[8 * BM + 1] = make_uint4(0u, 0u, 0u, 0u);
  }
  // VAR & 8 (round 4, measured A/B): static priority for the second-dispatched half of an 8-wave workgroup (cdna_hip_programming.md T5,
  // static form: the younger waves lose the issue arbitration on every segment)
  if ((VAR & 8) && NWM == 4 && wave >= 4) __builtin_amdgcn_s_setprio(1);
  // prologue: group 0 and the weight tiles of taps 0, 1 (BST == 2: of tap 0)
  dma_a(0, sA0);
  dma_b(0, 0, sB0);
  if constexpr (BST == 3) {
    dma_b(0, 1, sB1);
    tap_end(std::integral_constant<int, 2>{});
  } else {
    tap_end(std::integral_constant<int, 0>{});
  }
  for (int g = 0; g < G; g += 2) {
    group(g, c0);
    if (g + 1 >= G) break;
    group(g + 1, c1);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the look-ahead loads of a group that never comes: landed before LDS is reused
  __syncthreads();
  // (NWM == 2: a gathered stage holds 16 KB, so the epilogue stages 32 rows at a time)
  epilogue3<TM, TN, OP, 4, false, true, false, NWM, 128 * NWM, (NWM == 2 ? 1 : 0)>(p, acc, sA0, m0, n0, tid, wm, wn, il, h, g_bias, g_addend, g_mask, g_out, g_ohi, g_olo);
}

}  // namespace

void PP_API(pp3_launch_igemm4x)(hipStream_t st, const IgemmParams& p, const Igemm3Args& a, const PpIgemmPlan& pl) {
  const unsigned a_bytes = (unsigned)(p.src_rows * (long long)p.ld_src * 4), w_bytes = (unsigned)((long long)p.w_taps * a.w_rows * a.w_ld8 * 16);
  auto go = [&](auto var, auto nwm) {  // (NWM waves along the rows: 128 NWM threads)
    constexpr int VAR = decltype(var)::value, NWM = decltype(nwm)::value;
    hipLaunchKernelGGL((igemm4x_kernel<true, VAR, NWM>), dim3(pl.grid), dim3(128 * NWM), 0, st, p, a.ahi, a.alo, a_bytes, a.whi, a.wlo, w_bytes, p.bias,
                       p.addend, p.mask_src, p.out, (uint2*)a.ohi, (uint2*)a.olo, a.w_rows, a.w_ld8);
  };
  const std::integral_constant<int, 4> w4{};
  if (pl.family == PP_IGEMM4X2) go(std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{});
  else if (pl.variant == 0) go(std::integral_constant<int, 0>{}, w4);
  else if (pl.variant == 2) go(std::integral_constant<int, 2>{}, w4);
  else if (pl.variant == 3) go(std::integral_constant<int, 3>{}, w4);
  else if (pl.variant == 4) go(std::integral_constant<int, 4>{}, w4);
  else if (pl.variant == 9) go(std::integral_constant<int, 9>{}, w4);
  else go(std::integral_constant<int, 1>{}, w4);
}
