// Launch policy of the convolution kernels (conv.hip, the conv3 units, conv4.hip) as plain host C++: the PP_* switches, the facts a
// decision reads, and the plans -- which kernel family runs, with which tile, reduction split, grid and scratch use.  Nothing here
// needs the HIP runtime: the entry points fill the facts, call a planner and hand the plan to a launch function that only
// launches; pp_conv_plan_text does the same without a context, so the policy can be tested on a machine without a GPU.
// DESIGN.md ("Conv switches") is the table of every switch below.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

// ---- the switches ----
// Read ONCE, on the first use of any of them (an opt-in branch never freezes a value half way through a process any more).
struct PpConvSwitches {
  int gscale_log2;          // PP_GSCALE_LOG2: base of the gradient scale 2^G, clamped to [-20, 30] (8)
  bool fast;                // PP_CONV3_FAST: the branch-free igemm3f / wgrad3f loops (on)
  bool xreuse;              // PP_CONV3_XREUSE: the tap-row-reuse kernel igemm3x (on)
  int sparse_dgrad_splits;  // PP_SPARSE_DGRAD_SPLITS: reduction split of the listed-block launch (2)
  int sparse_dgrad;         // PP_SPARSE_DGRAD: 22 / 12 = tile of the listed-block launch, 0 = dense grid (22)
  int x_order;              // PP_CONV3_X_ORDER: loop order of igemm3x's (kernel row, channel chunk) groups (1)
  int dma_min;              // PP_CONV3_DMA_MIN: fewest 256 x 128 tiles for igemm4x (512 = two rounds)
  int dma_frac;             // PP_CONV3_DMA_FRAC: percent of a second round that also qualifies (1000 = never)
  bool dma_tail;            // PP_CONV3_DMA_TAIL: split a partly filled last round off into an igemm3x launch (on)
  int dma_tail_frac;        // PP_CONV3_DMA_TAIL_FRAC: percent below which the last round counts as partly filled (60)
  bool x4;                  // PP_CONV3_X4: keep the 256 x 128 tile where the row-reuse kernel applies (off)
  bool s2_classes;          // PP_CONV3_S2CLASSES: stride-2 data gradient as four parity-class launches (on)
  int wgrad3w_min;          // PP_WGRAD3W_MIN: channels from which the P16 weight gradient defaults to wgrad3w (512)
  int wgrad3_sp_steps;      // PP_WGRAD3_SP_STEPS: listed blocks one workgroup should at least reduce (1)
};
inline int pp_env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
inline bool pp_env_not0(const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); }
inline bool pp_env_is1(const char* name) { const char* e = getenv(name); return e && e[0] == '1'; }
inline const PpConvSwitches& pp_conv_switches() {
  static const PpConvSwitches s = []() {
    PpConvSwitches v;
    const int g = pp_env_int("PP_GSCALE_LOG2", 8);
    v.gscale_log2 = g < -20 ? -20 : (g > 30 ? 30 : g);
    v.fast = pp_env_not0("PP_CONV3_FAST");
    v.xreuse = pp_env_not0("PP_CONV3_XREUSE");
    v.sparse_dgrad_splits = pp_env_int("PP_SPARSE_DGRAD_SPLITS", 2);
    v.sparse_dgrad = pp_env_int("PP_SPARSE_DGRAD", 22);
    v.x_order = pp_env_int("PP_CONV3_X_ORDER", 1);
    v.dma_min = pp_env_int("PP_CONV3_DMA_MIN", 512);
    v.dma_frac = pp_env_int("PP_CONV3_DMA_FRAC", 1000);
    v.dma_tail = pp_env_not0("PP_CONV3_DMA_TAIL");
    v.dma_tail_frac = pp_env_int("PP_CONV3_DMA_TAIL_FRAC", 60);
    v.x4 = pp_env_is1("PP_CONV3_X4");
    v.s2_classes = pp_env_not0("PP_CONV3_S2CLASSES");
    const int wm = pp_env_int("PP_WGRAD3W_MIN", 0);
    v.wgrad3w_min = wm > 0 ? wm : 512;
    const int ss = pp_env_int("PP_WGRAD3_SP_STEPS", 0);
    v.wgrad3_sp_steps = ss > 0 ? ss : 1;
    return v;
  }();
  return s;
}
// Read at EVERY launch: tests and tools/conv_bench.py compare two kernels inside one process.
inline bool pp_sw_debug() { return getenv("PP_CONV_DEBUG") != nullptr; }
inline bool pp_sw_dma() { return pp_env_not0("PP_CONV3_DMA"); }            // igemm4x where it applies (on)
inline int pp_sw_dma_var() { return pp_env_int("PP_CONV3_DMA_VAR", 1); }   // its scheduling variant
inline bool pp_sw_dma2() { return pp_env_is1("PP_CONV3_DMA2"); }           // igemm4x<NWM=2> (off)
inline int pp_sw_dma2_min() { return pp_env_int("PP_CONV3_DMA2_MIN", 512); }  // (only looked at behind PP_CONV3_DMA2=1)
inline bool pp_sw_conv4p() { return pp_env_is1("PP_CONV4P"); }             // igemm4p for the 1x1 convolutions (off)
inline int pp_sw_conv4p_nst() { const char* e = getenv("PP_CONV4P_NST"); return e && atoi(e) == 3 ? 3 : 4; }
inline int pp_sw_conv4p_splits() { return pp_env_int("PP_CONV4P_SPLITS", 0); }
inline bool pp_sw_wgrad_det() { return pp_env_is1("PP_WGRAD3_DETERMINISTIC"); }
// PP_CONV3_S2MERGED (on): the engine's stride-2 data gradients go through pp_conv2d_nhwc_bwd_data_s2_bf16x3 (one launch for all
// parity classes); 0 = through pp_conv2d_nhwc_bwd_data_bf16x3 (one launch per class).  Read whenever a backward plan is built
// (pp_conv_s2_merged): the A/B and the bit-identity test build both plans in one process.  Neither entry point looks at it.
inline bool pp_sw_s2_merged() { return pp_env_not0("PP_CONV3_S2MERGED"); }
// PP_WGRAD3R: -1 unset, else its first character's digit (0 / 1 / 2; anything else counts as 0)
inline int pp_sw_wgrad3r() { const char* e = getenv("PP_WGRAD3R"); return !e ? -1 : ((e[0] == '1' || e[0] == '2') ? e[0] - '0' : 0); }
// "tm,tn" tuning hooks (PP_CONV_TILE, PP_CONV3_TILE, PP_WGRAD3_TILE): the two characters, or false
inline bool pp_sw_tile(const char* name, char* a, char* b) {
  const char* e = getenv(name);
  if (!(e && e[0] && e[1] == ',' && e[2])) return false;
  *a = e[0];
  *b = e[2];
  return true;
}
// forced split counts (PP_CONV3_SPLITS, PP_WGRAD3_SPLITS, PP_WGRAD3R_SPLITS): 0 when unset
inline int pp_sw_splits(const char* name) { const char* e = getenv(name); return e ? atoi(e) : 0; }

inline int pp_cus(int n_cu) { return n_cu > 0 ? n_cu : 256; }

// ---- launch-shape cost model (measured with tools/conv_bench.py on MI355X; DESIGN.md §Tile choice) ----
// A CU that holds c equal workgroups retires them at a relative MFMA rate thr(c) (one 4-wave workgroup per CU
// cannot hide its own staging latency: 0.62; four: 0.82 of the f32-MFMA peak).  Equal-length workgroups
// finish in lock-step rounds, so  time / L = full_rounds * S / thr(S) + c_tail / thr(c_tail)  with S the
// co-resident slots per CU, c_tail = ceil(remainder / CUs) and L the time of one workgroup alone at full rate.
inline double est_rounds(long long blocks, int slots, int cus) {
  static const double thr[5] = {1.0, 0.62, 0.78, 0.81, 0.82};
  const long long per_round = (long long)cus * slots;
  const long long full = blocks / per_round;
  const long long rem = blocks - full * per_round;
  const int s_idx = slots < 4 ? slots : 4;
  double t = (double)full * slots / thr[s_idx];
  if (rem > 0) {
    const int c = (int)((rem + cus - 1) / cus);
    t += (double)c / thr[c < 4 ? c : 4];
  }
  return t;
}

// workgroups of a split-K finishing pass over `rows` output rows (grid-stride, at most eight per CU)
inline unsigned pp_finish_blocks(long long rows, int Nout, int n_cu) {
  const long long total = rows * ((Nout + 3) >> 2);
  long long blocks = (total + 255) / 256;
  if (blocks > (long long)n_cu * 8) blocks = (long long)n_cu * 8;
  return (unsigned)blocks;
}

// ---- forward / data-gradient launches (conv3_igemm.hip: igemm3*, conv3_igemm4x.hip: igemm4x, conv4.hip: igemm4p) ----
struct PpIgemmFacts {
  // the shape (IgemmParams)
  int M, Nout, Cred, kh, kw, ld_out, ld_src, w_rows, w_ld8, w_taps, div, mul, sc_on, w_tstep, w_tx0;
  long long src_rows;
  int max_sw;      // widest level of the gathered tensor
  bool same_grid;  // every level: enumerated grid == gathered grid ("same" convolution)
  // the operand forms
  bool planes_in, f32_in, planes_out, f32_out, capture, flags;
  bool listed;     // launch over the LISTED 32-row blocks (sparse data gradient, pp_conv_opts.out_flags)
  int listed_tm;   // its tile: 2 (128 x 128) or 1 (64 x 128)
  // the resources
  int n_cu;        // already through pp_cus
  bool ws;
  long long ws_bytes;
};

enum PpIgemmFamily {
  PP_IGEMM3, PP_IGEMM3F, PP_IGEMM3F_CLASS, PP_IGEMM3X_CAPTURE, PP_IGEMM3X_PP, PP_IGEMM3X_PF, PP_IGEMM3X_FP, PP_IGEMM3X_FF, PP_IGEMM4X,
  PP_IGEMM4X2, PP_IGEMM4P, PP_IGEMM3F_LIST, PP_IGEMM3F_S2
};
static const char* const pp_igemm_family_name[] = {
    "igemm3", "igemm3f", "igemm3f[parity class]", "igemm3x[capture]", "igemm3x[planes->planes]", "igemm3x[planes->f32]",
    "igemm3x[f32->planes]", "igemm3x[f32->f32]", "igemm4x", "igemm4x<NWM=2>", "igemm4p", "igemm3f[row list]", "igemm3f[stride-2 merged]"};

struct PpIgemmPlan {
  int family;
  int tm, tn, splits;  // tile 64 tm x 64 tn; reduction split of the (main) launch
  int n_tiles_n;
  unsigned grid;
  int x_ty_inner, skip_halo;         // igemm3x / igemm4x
  int full_rt, tail_splits, variant; // igemm4x: 254-row tile rows it takes; split of the igemm3x launch over the rest (0: none)
  int tail_m_off;
  unsigned tail_grid;
  int stages;                        // igemm4p: stages of its ring (its grid: one persistent workgroup per CU, or per item if fewer)
  bool capture_first;                // split_capture_pass before the launch
  unsigned finish_blocks;            // split-K finish after the launch (0: none); over the tail's rows for igemm4x
  long long ws_need;                 // scratch bytes the plan writes
  int n_steps;
  bool may_split;
};

// the branch-free loop needs a tap-linear gather and 31-bit byte offsets (see igemm3f_kernel)
inline bool pp_igemm_fast_ok(const PpIgemmFacts& f) {
  const long long a_bytes = f.src_rows * (long long)f.ld_src * 4;  // (packed planes take the same 4 bytes per element)
  const long long w_bytes = (long long)f.w_taps * f.w_rows * f.w_ld8 * 16;
  return pp_conv_switches().fast && f.div == 1 && f.kh * f.kw <= 31 && a_bytes < (1ll << 31) && w_bytes < (1ll << 31) &&
         (long long)f.max_sw * f.ld_src * 4 < (1ll << 23) && f.src_rows > 0;
}

// the tap-row-reuse kernel applies: 3-wide stride-1 "same" geometry on an f32 operand (conditions of igemm3x_kernel)
inline bool pp_igemm_x_ok(const PpIgemmFacts& f) {
  return pp_conv_switches().xreuse && pp_igemm_fast_ok(f) && !f.sc_on && f.kw == 3 && f.mul == 1 && f.div == 1 && (f.f32_in || f.planes_in) &&
         (!f.planes_in || f.ld_src % 8 == 0) && f.w_tstep == 1 && f.w_tx0 == 0 && f.same_grid;
}

inline void pp_pick_tile3(const PpIgemmFacts& f, int n_steps, bool may_split, bool x_ok, int* tm, int* tn, int* splits) {
  // measured in-flight rates relative to 128x128 (tools/conv_bench.py): the LDS store path (ds_write_b128 of the
  // staged tiles) costs ~30 % of the loop, so the tile with the fewest staged bytes per MFMA wins when it fills the chip.
  // A workgroup costs (its k-steps + ~8 steps' worth of prologue, epilogue and launch ramp) x tile area; splitting the
  // reduction S ways multiplies the workgroups and pays S x the output in f32 atomics plus the finishing pass.
  static const int cand[5][2] = {{4, 2}, {2, 2}, {1, 2}, {2, 1}, {1, 1}};
  static const double eff[5] = {1.1, 1.0, 0.9, 0.9, 0.8};
  static const int slots[5] = {2, 3, 4, 4, 4};
  static const int split_cand[8] = {1, 2, 3, 4, 6, 8, 12, 16};
  const int M = f.M, Nout = f.Nout, ld_out = f.ld_out, cus = f.n_cu;
  const long long ws_bytes = f.ws_bytes;
  double best = 1e300;
  *splits = 1;
  for (int i = 0; i < 5; ++i) {
    const int bm = 64 * cand[i][0], bn = 64 * cand[i][1];
    const long long blocks = (long long)((M + bm - 1) / bm) * ((Nout + bn - 1) / bn);
    for (int si = 0; si < (may_split ? 8 : 1); ++si) {
      const int sp = split_cand[si];
      if (sp > 1 && (n_steps / sp < 8 || (long long)sp * M * ld_out * 4 > ws_bytes)) break;
      const double steps = (double)((n_steps + sp - 1) / sp) + 8.0;
      double t = est_rounds(blocks * sp, slots[i], cus) * steps * cand[i][0] * cand[i][1] / eff[i];
      if (sp > 1) {
        // slices: sp x M x N x 4 B written and read back (~4 TB/s), the epilogue operands, one more launch; one k-step
        // of a 128x128 tile ~ 2.1 us when the chip is full  ->  convert microseconds to the same step units
        const double us = (double)M * Nout * (8.0 * sp + 12.0) / 4.0e6 + 4.0;
        t += us / 2.1 * 4.0;
      }
      if (t < best * 0.97) {
        best = t;
        *tm = cand[i][0];
        *tn = cand[i][1];
        *splits = sp;
      }
    }
  }
  // the 256x128 tile has no tap-row-reuse variant: where that kernel applies, 128x128 with reuse wins (measured on the
  // 256-channel class head, 50400 rows: 194-207 us against 205-227 us; a reuse bonus inside the model above instead sent
  // that shape to 64x128 and the step lost 2 %)
  if (x_ok && *tm == 4 && *splits == 1 && !pp_conv_switches().x4) {
    *tm = 2;
    *tn = 2;
  }
  char a, b;
  if (pp_sw_tile("PP_CONV3_TILE", &a, &b)) {
    *tm = a - '0';
    *tn = b - '0';
  }
  if (const int v = pp_sw_splits("PP_CONV3_SPLITS")) {
    if (v >= 1 && (v == 1 || (may_split && n_steps / v >= 1 && (long long)v * M * ld_out * 4 <= ws_bytes))) *splits = v;
  }
  // the launch functions exist for these five tiles; anything else a PP_CONV3_TILE asks for runs (and now prints) as the tile it
  // always ran as: 256 x 128 for tm = 4, 64 x 64 otherwise
  if (*tm == 4) *tn = 2;
  else if (!((*tm == 2 || *tm == 1) && (*tn == 2 || *tn == 1))) *tm = *tn = 1;
}

// The sparse data gradient / forward over the listed blocks.  The listed tiles are few (a fifth of the rows on the bench targets:
// ~320 workgroups of 144 k-steps each on 256 CUs, every one of them alone with its load latencies): with a scratch buffer the
// reduction is split two ways (PP_SPARSE_DGRAD_SPLITS) and rl_splitk_finish_kernel adds the slices of the listed blocks.
inline void pp_plan_listed(const PpIgemmFacts& f, PpIgemmPlan* pl) {
  const int nb = (f.M + 31) / 32, BM = 64 * f.listed_tm, BN = 128;
  const int want_splits = pp_conv_switches().sparse_dgrad_splits;
  int splits = 1;
  if (f.ws && want_splits > 1 && (f.planes_out || f.f32_out)) {
    const long long slice_bytes = (long long)nb * 32 * f.ld_out * 4;
    splits = want_splits;
    while (splits > 1 && (pl->n_steps / splits < 24 || slice_bytes * splits > f.ws_bytes)) --splits;
  }
  pl->family = PP_IGEMM3F_LIST;
  pl->tm = f.listed_tm;
  pl->tn = 2;
  pl->splits = splits;
  pl->n_tiles_n = (f.Nout + BN - 1) / BN;
  pl->grid = (unsigned)(((nb + BM / 32 - 1) / (BM / 32)) * pl->n_tiles_n * splits);
  pl->finish_blocks = splits > 1 ? (unsigned)nb : 0u;
  pl->ws_need = splits > 1 ? (long long)nb * 32 * f.ld_out * 4 * splits : 0;
}

inline PpIgemmPlan pp_plan_igemm(const PpIgemmFacts& f) {
  const PpConvSwitches& sw = pp_conv_switches();
  PpIgemmPlan pl = {};
  const int n_steps = pl.n_steps = f.kh * f.kw * (f.Cred / 32);
  const int n_cu = f.n_cu;
  if (f.listed) {
    pp_plan_listed(f, &pl);
    return pl;
  }
  // Round 4: 1x1 convolutions on plane-stored operands (the bottleneck branches of the backbone, the FPN laterals; forward and
  // stride-1 data gradient) -> the persistent LDS-DMA GEMM of conv4.hip.  OPT-IN (PP_CONV4P=1): bit-identical, but 1.05-1.9x
  // SLOWER than igemm3f per launch and -7 % on the training step (profiles/r04_1x1_persistent_dma_gemm.txt);
  // PP_CONV4P_NST: stages of its ring (4 = all of the CU's LDS, default; 3); PP_CONV4P_SPLITS forces the reduction split.
  // (read at every launch: tests compare the two kernels inside one process)
  // (off by default: measured slower than igemm3f on every backbone shape, see conv4.hip)
  if (pp_sw_conv4p()) {
    const long long a_bytes = f.src_rows * (long long)f.ld_src * 4, w_bytes = (long long)f.w_taps * f.w_rows * f.w_ld8 * 16;
    if (f.kh == 1 && f.kw == 1 && f.planes_in && !f.capture && !f.flags && !f.sc_on && f.div == 1 && f.Cred % 32 == 0 && f.ld_src % 8 == 0 &&
        a_bytes < (1ll << 31) && w_bytes < (1ll << 31) && f.src_rows > 0 && (f.planes_out || f.f32_out)) {
      const int p_splits = pp_sw_conv4p_splits();
      const long long tiles = (long long)((f.M + 127) / 128) * ((f.Nout + 127) / 128);
      int sp = 1;
      if (tiles * 4 < (long long)n_cu * 3 && f.ws) {  // under three quarters of a round: split the reduction to fill the chip
        sp = (int)(n_cu / tiles);
        while (sp > 1 && (n_steps / sp < 4 || (long long)sp * f.M * f.ld_out * 4 > f.ws_bytes)) --sp;
      }
      if (p_splits >= 1 && (p_splits == 1 || (f.ws && n_steps / p_splits >= 1 && (long long)p_splits * f.M * f.ld_out * 4 <= f.ws_bytes)))
        sp = p_splits;
      pl.family = PP_IGEMM4P;
      pl.tm = pl.tn = 2;
      pl.splits = sp;
      pl.stages = pp_sw_conv4p_nst();
      pl.n_tiles_n = (f.Nout + 127) / 128;
      const long long n_items = tiles * sp;
      pl.grid = (unsigned)(n_items < n_cu ? n_items : n_cu);
      pl.finish_blocks = sp > 1 ? pp_finish_blocks(f.M, f.Nout, n_cu) : 0u;
      pl.ws_need = sp > 1 ? (long long)sp * f.M * f.ld_out * 4 : 0;
      return pl;
    }
  }
  const bool fast = pp_igemm_fast_ok(f), x_ok = pp_igemm_x_ok(f);
  const bool may_split = pl.may_split = f.ws && (f.planes_out || f.f32_out) && !f.sc_on && fast;
  int tm = 1, tn = 1, splits = 1;
  pp_pick_tile3(f, n_steps, may_split, x_ok, &tm, &tn, &splits);
  pl.tm = tm;
  pl.tn = tn;
  pl.splits = splits;
  const int BM = 64 * tm, BN = 64 * tn;
  pl.n_tiles_n = (f.Nout + BN - 1) / BN;
  pl.grid = (unsigned)(((f.M + BM - 1) / BM) * pl.n_tiles_n * splits);
  pl.finish_blocks = splits > 1 ? pp_finish_blocks(f.M, f.Nout, n_cu) : 0u;
  pl.ws_need = splits > 1 ? (long long)splits * f.M * f.ld_out * 4 : 0;
  if (f.sc_on) {  // parity-class launch of a stride-2 bwd-data (host guarantees: fast, no split, planes on both sides or on neither)
    pl.family = PP_IGEMM3F_CLASS;
    return pl;
  }
  // (the 256-row tile has the tap-row-reuse kernel for plane-stored operands only: its f32 form would need 32 more staging registers)
  if (x_ok && (tm <= 2 || (f.planes_in && !f.capture))) {
    const int n_tiles_mx = (f.M + BM - 3) / (BM - 2);  // tiles overlap by two rows
    pl.skip_halo = f.max_sw + 1;
    pl.grid = (unsigned)(n_tiles_mx * pl.n_tiles_n * splits);
    pl.x_ty_inner = sw.x_order;
    // with split-K the partial sums go to the f32 scratch and splitk_finish_kernel writes the output (planes included)
    const bool op = f.planes_out && splits == 1;
    if (tm <= 2 && f.capture) {  // the capture inside the kernel (f32 operand)
      pl.family = PP_IGEMM3X_CAPTURE;
      return pl;
    }
    // the multi-stage LDS-DMA form of this launch (igemm4x_kernel: planes in and out, at least two rounds of 256 x 128 tiles);
    // PP_CONV3_DMA=0 keeps everything on igemm3x
    // (read at every launch, unlike the other knobs: tests compare the two kernels inside one process)
    if (tm == 2 && tn == 2 && pp_sw_dma() && f.planes_in && op && !f.flags && splits == 1 && f.kh == 3 && sw.x_order == 1 && f.w_rows % 128 == 0 &&
        f.Cred % 32 == 0) {
      const int BM4 = 256;
      const int n_tiles_m4 = (f.M + BM4 - 3) / (BM4 - 2);
      const int ntn = (f.Nout + 127) / 128;
      // (one workgroup per CU: a launch of less than two rounds is better off with three 128 x 128 workgroups per CU)
      // between one and two rounds (the 256-channel heads: 398 tiles) one launch CAN pay in isolation when the second round is
      // at least half full (PP_CONV3_DMA_FRAC=50: class head 149 us against 162; 1.19 rounds do not: mask head 137 / 115) -- but in
      // the training step those launches run beside the regression head's on the other lane, and two 115 KB workgroups cannot
      // share a CU where a 33 KB one fits next to this kernel's: the step LOSES 2.4 % (594 vs 608 images/s).  Off by default.
      const int n_blk = n_tiles_m4 * ntn;
      const bool one_and_a_bit = n_blk > n_cu && n_blk < 2 * n_cu && (n_blk - n_cu) * 100 >= sw.dma_frac * n_cu;
      if (n_blk >= sw.dma_min || one_and_a_bit) {
        // Whole rounds of 256 x 128 tiles go to igemm4x; with one workgroup per CU a last, partly filled round would cost a
        // full round's time, so the rows of that round are a second launch: 128 x 128 tiles of igemm3x with the reduction
        // split over enough workgroups to fill the chip once (partial sums -> scratch, splitk_finish_kernel writes the rows)
        int full_rt = n_tiles_m4;
        const int rounds = (n_tiles_m4 * ntn) / n_cu;
        // (a last round that is mostly full stays in the one launch: 720 x 540 gives 1 016 tiles = 3.97 rounds)
        const int last = (n_tiles_m4 * ntn) % n_cu;
        if (sw.dma_tail && last != 0 && last * 100 < sw.dma_tail_frac * n_cu && rounds >= 2 && f.ws) full_rt = rounds * n_cu / ntn;
        const int m_split = full_rt * (BM4 - 2);
        int tail_splits = 0;
        if (full_rt < n_tiles_m4) {
          const int rem = f.M - m_split;
          const int n_rt = (rem + BM - 3) / (BM - 2);
          const int groups = f.kh * (f.Cred / 32);
          int sp = (3 * n_cu + n_rt * ntn - 1) / (n_rt * ntn);  // ~ one full round of three workgroups per CU
          while (sp > 1 && (groups / sp < 4 || (long long)sp * rem * f.ld_out * 4 > f.ws_bytes)) --sp;
          if (sp > 1) tail_splits = sp;
          else full_rt = n_tiles_m4;  // (no room to split: everything in the one launch)
        }
        // scheduling variants (measured on the regression-head launch, P16): 1 = no iglp_opt hint in the k-step (default: 442 us
        // against 465 with igemm3x's hint, 0), 2 / 3 = s_setprio around the MFMAs of 0 / 1 (466 / 461), 4 = igemm3f's sched_barrier
        // (per launch: A/B in one process).  The figures of 0 and 2 are of the build that had igemm4x in one unit with igemm3x: as a unit
        // of its own the two hinted variants compile to other register counts (profiles/conv3_split_kernel_resources.txt), not re-timed
        const int var = pp_sw_dma_var();
        pl.family = PP_IGEMM4X;
        pl.variant = (var == 0 || var == 2 || var == 3 || var == 4 || var == 9) ? var : 1;
        pl.n_tiles_n = ntn;
        pl.full_rt = full_rt;
        pl.grid = (unsigned)(full_rt * ntn);
        pl.tail_splits = tail_splits;
        if (tail_splits > 1) {
          const int rem = f.M - full_rt * (BM4 - 2);
          pl.tail_m_off = full_rt * (BM4 - 2);
          pl.tail_grid = (unsigned)(((rem + BM - 3) / (BM - 2)) * ntn * tail_splits);
          pl.finish_blocks = pp_finish_blocks(rem, f.Nout, n_cu);
          pl.ws_need = (long long)tail_splits * rem * f.ld_out * 4;
        }
        return pl;
      }
      // Round 4: launches too small for two rounds of 256-row tiles (the 256-channel heads, the FPN 3x3: 1.2-1.6 rounds of 128-row
      // tiles on 2 x 256 slots) CAN take the 128 x 128 form of the same pipeline, two workgroups per CU (PP_CONV3_DMA2=1: opt-in;
      // PP_CONV3_DMA2_MIN: fewest 128-row tiles, default one round; both per launch, like PP_CONV3_DMA)
      // (off by default: +8 % on the class-head launch, -8 % on the mask head / FPN launches -- 610 tiles on 512 slots --, -2 % on
      // the training step, profiles/r04_lds_dma_128_row_tiles.txt)
      if (pp_sw_dma2() && n_tiles_mx * ntn >= pp_sw_dma2_min()) {
        pl.family = PP_IGEMM4X2;
        pl.n_tiles_n = ntn;
        pl.grid = (unsigned)(n_tiles_mx * ntn);
        return pl;
      }
    }
    pl.family = f.planes_in ? (op ? PP_IGEMM3X_PP : PP_IGEMM3X_PF) : (op ? PP_IGEMM3X_FP : PP_IGEMM3X_FF);
    return pl;
  }
  pl.capture_first = f.capture;
  pl.family = fast ? PP_IGEMM3F : PP_IGEMM3;
  return pl;
}

// ---- which launches a data gradient is made of ----
struct PpDgradRouteFacts {
  int stride, kh, kw, pad_t, pad_l, n_seg;
  bool all_f32, all_planes, capture, bias, skip, skip_scratch, fast_ok, same_grid;
};
// Row-block skip: does the launch over the LISTED blocks apply?  PP_SPARSE_DGRAD: 22 (default) / 12 = tile of that launch (equal
// within noise on the bench step), 0 = keep the dense grid and skip the k-loop of tiles that see no flagged block (coarser: a
// 126-row tile spans 1.6 image rows)
inline bool pp_dgrad_listed_ok(const PpDgradRouteFacts& r) {
  return r.skip && r.skip_scratch && pp_conv_switches().sparse_dgrad && (r.all_f32 || r.all_planes) && !r.capture && r.stride == 1 && r.kh == 3 &&
         r.kw == 3 && r.pad_t == 1 && r.pad_l == 1 && !r.bias && r.fast_ok && r.same_grid;
}
// stride 2 as four stride-1 launches, one per parity class of the input grid (the parity-class / row-list kernels exist for
// all-f32 and all-planes operands)
inline bool pp_dgrad_classes_ok(const PpDgradRouteFacts& r) {
  return r.stride == 2 && pp_conv_switches().s2_classes && (r.all_f32 || r.all_planes) && r.n_seg == 1;
}

// ---- the parity classes of a stride-2 data gradient, and their merged launch (pp_conv2d_nhwc_bwd_data_s2_bf16x3) ----
// Input cell (2y' + cy, 2x' + cx) only receives the taps ty = ty0 + 2i with ty0 = (cy + pad_t) & 1 (x alike), from output cell
// y' + (cy + pad_t - ty0) / 2 - i: class (cy, cx) is a stride-1 gather of kh x kw taps over its own OH x OW grid.
struct PpS2Class {
  int cy, cx;                        // the class
  int kh, kw;                        // its taps (0 x 0: none -- the class only runs the epilogue)
  int off_y, off_x, w_ty0, w_tx0;    // gather offset; first weight tap (the weight taps step by 2)
  int OH, OW, M;                     // the class grid; its rows over all images (0: the class does not exist)
  int tiles, blk_begin;              // merged launch: workgroups of the class, and the first of them in the grid
};
// cls[2 * cy + cx]
inline void pp_s2_classes(int n_img, int H, int W, int kh, int kw, int pad_t, int pad_l, PpS2Class cls[4]) {
  for (int c = 0; c < 4; ++c) {
    PpS2Class& r = cls[c];
    r.cy = c >> 1;
    r.cx = c & 1;
    const int ty0 = (r.cy + pad_t) & 1, tx0 = (r.cx + pad_l) & 1;
    r.kh = ty0 < kh ? (kh - ty0 + 1) / 2 : 0;
    r.kw = tx0 < kw ? (kw - tx0 + 1) / 2 : 0;
    r.off_y = (r.cy + pad_t - ty0) / 2;
    r.off_x = (r.cx + pad_l - tx0) / 2;
    r.w_ty0 = ty0;
    r.w_tx0 = tx0;
    if (r.kh == 0 || r.kw == 0) r.kh = r.kw = 0;
    r.OH = (H - r.cy + 1) / 2;
    r.OW = (W - r.cx + 1) / 2;
    r.M = n_img * r.OH * r.OW;
    r.tiles = r.blk_begin = 0;
  }
}
// The merged launch: the tile grids of the classes that have rows, one behind the other, the class with the most taps first (4, 2,
// 2, 1, 0 for a 3x3 kernel: the light tiles fill the last round); a workgroup finds its class by comparing its index with
// c[1 ..].blk_begin.  Passed to the kernel by value.
struct PpS2Merged {
  int n_cls;
  unsigned grid;
  PpS2Class c[4];
};
inline PpS2Merged pp_s2_merge(const PpS2Class cls[4], int BM, int BN, int Nout) {
  PpS2Merged g = {};
  for (int c = 0; c < 4; ++c) {
    if (cls[c].M <= 0) continue;
    int at = g.n_cls++;
    for (; at > 0 && g.c[at - 1].kh * g.c[at - 1].kw < cls[c].kh * cls[c].kw; --at) g.c[at] = g.c[at - 1];  // stable: ties keep class order
    g.c[at] = cls[c];
  }
  const long long ntn = (Nout + BN - 1) / BN;
  long long at = 0;
  for (int i = 0; i < g.n_cls; ++i) {
    g.c[i].tiles = (int)(((g.c[i].M + BM - 1) / BM) * ntn);
    g.c[i].blk_begin = (int)at;
    at += g.c[i].tiles;
  }
  g.grid = (unsigned)at;
  return g;
}
// the route applies to what the per-class route applies to (the entry point refuses everything else: no fall-back)
inline bool pp_dgrad_s2_ok(const PpDgradRouteFacts& r) { return r.stride == 2 && (r.all_f32 || r.all_planes) && r.n_seg == 1; }

// ---- weight-gradient launches (conv3_wgrad.hip: wgrad3 / wgrad3f, conv4.hip: wgrad3r / wgrad3w) ----
struct PpWgradFacts {
  int M, Cin, Cout, kh, kw, stride, pad_t, pad_l, ld_src, ld_dy, ld_w;
  long long src_rows;
  int min_ow, min_hw;        // narrowest level, smallest level (cells per image)
  bool same_grid;
  bool list_levels_aligned;  // every level but the first begins on a 32-row block
  long long Mp;              // wgrad3r's position space: every image row followed by one pad
  bool planes, list, lazy_in;
  int fmt;                   // plane format 0 / 1
  int n_cu;
  bool ws;
  long long ws_bytes;
  bool dw_aligned, dbias_aligned;  // 16 bytes (dbias: or absent)
};

enum PpWgradFamily { PP_WGRAD3, PP_WGRAD3F_PLANES_LIST, PP_WGRAD3F_PLANES, PP_WGRAD3F_F32_LIST, PP_WGRAD3F_F32, PP_WGRAD3R, PP_WGRAD3W };
static const char* const pp_wgrad_family_name[] = {"wgrad3", "wgrad3f[planes, list]", "wgrad3f[planes]", "wgrad3f[f32, list]", "wgrad3f[f32]",
                                                   "wgrad3r", "wgrad3w"};

struct PpWgradPlan {
  int family;
  bool refused;  // dy was declared lazy but no listed-block reduction applies
  int tm, tn;
  bool fast;
  int k_tiles_per_tap, n_tiles_k, n_tiles_n, tiles;
  int model_splits;  // the cost model's pick, before the rows of a split are rounded up to 32
  int splits, rows_per_split, max_wraps, sp_min_steps;
  bool use_ws;
  long long ws_slice;  // floats of one slice
  unsigned grid, finish_blocks;
  long long ws_need;
};

// the tap-row-reuse weight gradient (wgrad3r / wgrad3w): false when the launch does not meet the kernels' conditions
inline bool pp_plan_wgrad3r(const PpWgradFacts& f, int variant, PpWgradPlan* pl) {
  if (!(f.kh == 3 && f.kw == 3 && f.stride == 1 && f.pad_t == 1 && f.pad_l == 1 && f.Cin % 128 == 0 && f.planes)) return false;
  if (variant == 2 && f.list) return false;  // wgrad3w: dense reductions only
  if (!f.same_grid) return false;
  if (f.list && !f.list_levels_aligned) return false;  // (a listed 32-row block never straddles two levels)
  const long long x_bytes = f.src_rows * (long long)f.ld_src * 4, d_bytes = (long long)f.M * f.ld_dy * 4;
  if (!(f.min_ow >= (f.list ? 12 : 2) && x_bytes < (1ll << 31) && d_bytes < (1ll << 31) && f.Mp < (1 << 24) && f.src_rows > 0)) return false;
  pl->k_tiles_per_tap = f.Cin / 128;
  pl->n_tiles_k = 3 * pl->k_tiles_per_tap;
  pl->n_tiles_n = (f.Cout + 127) / 128;
  const int tiles = pl->tiles = pl->n_tiles_k * pl->n_tiles_n;
  const int R = f.list ? f.M : (int)f.Mp;  // length of the reduction space
  // row splits: one workgroup per CU and ~1 us per 3-tap step; every split adds a |dW| of f32 atomics (~1.3 TB/s, about half of it
  // under other workgroups' loops)
  int max_splits = (R + 255) / 256;  // at least 8 steps per workgroup
  if (max_splits > 128) max_splits = 128;
  if (max_splits < 1) max_splits = 1;
  const double atomic_steps_per_split = 0.5 * (double)tiles * 3.0 * 128.0 * 128.0 * 4.0 / 1.3e6 / 1.0;
  int splits = 1;
  double best = 1e300;
  for (int sp = 1; sp <= max_splits; ++sp) {
    const double steps = (double)((R + sp - 1) / sp + 31) / 32.0 + 6.0;
    const double rounds = (double)(((long long)tiles * sp + f.n_cu - 1) / f.n_cu);
    const double cost = rounds * steps + atomic_steps_per_split * sp;
    if (cost < best * 0.995) {
      best = cost;
      splits = sp;
    }
  }
  if (const int v = pp_sw_splits("PP_WGRAD3R_SPLITS")) {
    if (v >= 1 && v <= max_splits) splits = v;
  }
  int rps = (R + splits - 1) / splits;
  rps = (rps + 31) / 32 * 32;
  splits = (R + rps - 1) / rps;
  pl->family = variant == 2 ? PP_WGRAD3W : PP_WGRAD3R;
  pl->tm = pl->tn = 2;
  pl->fast = true;
  pl->model_splits = pl->splits = splits;
  pl->rows_per_split = rps;
  pl->grid = (unsigned)(tiles * splits);
  return true;
}

inline PpWgradPlan pp_plan_wgrad(const PpWgradFacts& f) {
  const PpConvSwitches& sw = pp_conv_switches();
  PpWgradPlan pl = {};
  pl.sp_min_steps = sw.wgrad3_sp_steps;
  // one slice = a full-size copy of dW plus a bias row (f32).  PP_WGRAD3_DETERMINISTIC=1 (and a scratch buffer): the splits write
  // slices and a finishing pass adds them in a fixed order -- bit-reproducible gradients; default: float atomics into dW, which
  // are fire-and-forget and overlap the k-loops of other workgroups (measured in the training step, same box, slices vs
  // atomics: 531.5 vs 537.1 images/s, dense backward 424 vs 433: the extra pass and its launch cost more than the atomics)
  // (read per launch, like the choice of kernel below)
  const bool det = pp_sw_wgrad_det();
  {
    // Round 4: 3x3 stride-1 "same" layers on plane-stored operands -> the tap-row-reuse kernels of conv4.hip (one staged tile pair per
    // kernel ROW, 192 accumulators).  PP_WGRAD3R (read per launch: tests compare the kernels in one process):
    //   unset  wgrad3w (producer + consumer waves) for the DENSE reductions of the P16 launches with 512 input or output channels --
    //          the 3D-box head: 5-19 % faster per launch, +2.8 % on the dense-backward step; the 256-wide launches gain 5-13 % in
    //          isolation and LOSE 1 % in the step (a workgroup of 8 waves x 256 registers owns its CU: nothing of the data-gradient
    //          lane runs beside it), the bf16-pair launches of the backbone lose outright (profiles/r04_wgrad_producer_consumer_waves.txt);
    //          PP_WGRAD3W_MIN moves the channel threshold
    //   0      wgrad3f everywhere
    //   1      wgrad3r (one wave per SIMD; dense launches 1.15-1.45x SLOWER than wgrad3f: profiles/r04_wgrad_tap_row_reuse.txt)
    //   2      wgrad3w wherever its conditions hold
    // The deterministic slices mode keeps wgrad3f.
    const int e_r = pp_sw_wgrad3r();
    int variant = 0;
    if (e_r > 0) variant = e_r;
    else if (e_r < 0 && f.fmt == 1 && !f.list && (f.Cin >= sw.wgrad3w_min || f.Cout >= sw.wgrad3w_min)) variant = 2;
    if (variant && f.planes && !(det && f.ws) && (!f.lazy_in || f.list) && pp_plan_wgrad3r(f, variant, &pl)) return pl;
  }
  // (tools/sweep_wgrad.sh: the small 1x1 layers of res4 / res5 take ~35 us for ANY tile / split choice: ~19 latency-bound
  // steps of a lone workgroup per CU plus the f32 atomics of splits x |dW|.  Register double-buffering of the staged tiles
  // (loads two steps ahead) shortens such lone-workgroup launches by 10-20 % in isolation, but no measurable step time.)
  bool big_k = (f.Cin % 128 == 0);
  bool big_n = ((f.Cout + 127) / 128 * 128) <= ((f.Cout + 63) / 64 * 64);
  char a, b;
  if (pp_sw_tile("PP_WGRAD3_TILE", &a, &b)) {  // tuning hook: "1,1" / "1,2" / "2,1" / "2,2"
    big_k = big_k && a == '2';
    big_n = b == '2';
  }
  const int TM = pl.tm = big_k ? 2 : 1, TN = pl.tn = big_n ? 2 : 1;
  pl.max_wraps = (32 + f.min_ow - 1) / f.min_ow;
  const int BM = 64 * TM, BN = 64 * TN;
  pl.k_tiles_per_tap = f.Cin / BM;
  pl.n_tiles_k = f.kh * f.kw * pl.k_tiles_per_tap;
  pl.n_tiles_n = (f.Cout + BN - 1) / BN;
  const int tiles = pl.tiles = pl.n_tiles_k * pl.n_tiles_n;
  const int cus = f.n_cu;
  int max_splits = (f.M + 511) / 512;  // at least 16 reduction steps of 32 rows per workgroup
  if (max_splits < 1) max_splits = 1;
  if (max_splits > 64) max_splits = 64;
  const long long x_bytes = f.src_rows * (long long)f.ld_src * 4, d_bytes = (long long)f.M * f.ld_dy * 4;  // f32 or packed planes
  const bool fast = pl.fast = sw.fast && x_bytes < (1ll << 31) && d_bytes < (1ll << 31) && f.M < (1 << 24) && f.src_rows > 0 && f.min_hw >= 32;
  if (f.lazy_in && !(fast && f.list)) {  // (only the listed-block reduction never looks at the other rows of dy)
    pl.refused = true;
    return pl;
  }
  const int slots = fast ? ((TM * TN == 4) ? 3 : 4) : ((TM * TN == 4) ? 2 : 3);
  const double tile_work = (double)(TM * TN) / 4.0;
  const long long ws_slice = pl.ws_slice = (long long)f.kh * f.kw * f.Cin * f.ld_w + f.ld_w;
  const bool use_ws = pl.use_ws = fast && f.ws && f.ws_bytes >= ws_slice * 4 && f.dw_aligned && f.dbias_aligned && det;
  if (use_ws) {
    const long long fit = f.ws_bytes / (ws_slice * 4);
    if (max_splits > fit) max_splits = (int)fit;
  }
  // per split: atomics = |dW| at ~1.3 TB/s, half of it hidden under the k-loops of other workgroups (measured: 256-channel
  // head convs 252 -> 234 us going from 14 to 21 splits); slices = |dW| written and read back once at ~4 TB/s
  const double atomic_us_per_split = use_ws ? (double)tiles * BM * BN * 4.0 * 2.0 / 4.0e6 : 0.5 * (double)tiles * BM * BN * 4.0 / 1.3e6;
  int splits = 1;
  double best = 1e300;
  for (int sp = 1; sp <= max_splits; ++sp) {
    const double steps = (double)((f.M + sp - 1) / sp + 31) / 32.0;
    const double cost = est_rounds((long long)tiles * sp, slots, cus) * steps * tile_work * 0.8 + atomic_us_per_split * sp;
    if (cost < best * 0.995) {
      best = cost;
      splits = sp;
    }
  }
  if (const int v = pp_sw_splits("PP_WGRAD3_SPLITS")) {  // tuning hook
    if (v >= 1 && v <= max_splits) splits = v;
  }
  pl.model_splits = splits;
  int rps = (f.M + splits - 1) / splits;
  rps = (rps + 31) / 32 * 32;
  splits = (f.M + rps - 1) / rps;
  pl.splits = splits;
  pl.rows_per_split = rps;
  pl.grid = (unsigned)(tiles * splits);
  pl.family = !fast ? PP_WGRAD3
                    : (f.planes ? (f.list ? PP_WGRAD3F_PLANES_LIST : PP_WGRAD3F_PLANES) : (f.list ? PP_WGRAD3F_F32_LIST : PP_WGRAD3F_F32));
  if (use_ws && splits > 1) {  // (a single split adds its tile straight into dW)
    const long long n4 = (ws_slice - f.ld_w) / 4;
    long long blocks = (n4 + f.ld_w / 4 + 255) / 256;
    if (blocks > (long long)cus * 8) blocks = (long long)cus * 8;
    pl.finish_blocks = (unsigned)blocks;
    pl.ws_need = (long long)splits * ws_slice * 4;
  }
  return pl;
}

// ---- the PP_CONV_DEBUG lines: the only place that writes one.  detail: also the plan's numbers as key=value (pp_conv_plan_text) ----
inline int pp_plan_append(char* buf, int cap, int at, const char* fmt, ...) {
  if (at >= cap) return at;
  va_list ap;
  va_start(ap, fmt);
  const int n = vsnprintf(buf + at, (size_t)(cap - at), fmt, ap);
  va_end(ap);
  return n < 0 ? at : (at + n < cap ? at + n : cap);
}
inline int pp_plan_print(char* buf, int cap, int at, const PpIgemmFacts& f, const PpIgemmPlan& pl, bool detail) {
  if (pl.family == PP_IGEMM4P)
    at = pp_plan_append(buf, cap, at, "igemm4p M %d N %d steps %d -> %lld tiles x %d splits on %d CUs, %d stages", f.M, f.Nout, pl.n_steps,
                        (long long)((f.M + 127) / 128) * ((f.Nout + 127) / 128), pl.splits, f.n_cu, pl.stages);
  else if (pl.family == PP_IGEMM3F_LIST)
    at = pp_plan_append(buf, cap, at, "igemm3 M %d N %d steps %d -> tile %dx%d splits %d (listed blocks)", f.M, f.Nout, pl.n_steps, 64 * pl.tm,
                        64 * pl.tn, pl.splits);
  else
    at = pp_plan_append(buf, cap, at, "igemm3 M %d N %d steps %d -> tile %dx%d splits %d (may_split %d: ws %d planes_out %d out %d)", f.M, f.Nout,
                        pl.n_steps, 64 * pl.tm, 64 * pl.tn, pl.splits, (int)pl.may_split, (int)f.ws, (int)f.planes_out, (int)f.f32_out);
  at = pp_plan_append(buf, cap, at, " %s", pp_igemm_family_name[pl.family]);
  if (detail)
    at = pp_plan_append(buf, cap, at, " | grid=%u n_tiles_n=%d x_ty_inner=%d skip_halo=%d full_rt=%d tail_splits=%d tail_grid=%u tail_m_off=%d "
                        "variant=%d stages=%d capture_first=%d finish_blocks=%u ws_need=%lld",
                        pl.grid, pl.n_tiles_n, pl.x_ty_inner, pl.skip_halo, pl.full_rt, pl.tail_splits, pl.tail_grid, pl.tail_m_off, pl.variant,
                        pl.stages, (int)pl.capture_first, pl.finish_blocks, pl.ws_need);
  return pp_plan_append(buf, cap, at, "\n");
}
inline int pp_plan_print(char* buf, int cap, int at, const PpWgradFacts& f, const PpWgradPlan& pl, bool detail) {
  if (pl.refused) return pp_plan_append(buf, cap, at, "wgrad3 refused: lazy dy without a listed-block reduction\n");
  if (pl.family == PP_WGRAD3R || pl.family == PP_WGRAD3W)
    at = pp_plan_append(buf, cap, at, "wgrad3r tiles %d (3 taps each) splits %d (M %d)%s", pl.tiles, pl.splits, f.M, f.list ? " listed blocks" : "");
  else
    at = pp_plan_append(buf, cap, at, "wgrad3 tile %dx%d tiles %d splits %d (M %d) fast %d", 64 * pl.tm, 64 * pl.tn, pl.tiles, pl.model_splits, f.M,
                        (int)pl.fast);
  at = pp_plan_append(buf, cap, at, " %s", pp_wgrad_family_name[pl.family]);
  if (detail)
    at = pp_plan_append(buf, cap, at, " | grid=%u tile=%dx%d splits=%d rows_per_split=%d max_wraps=%d sp_min_steps=%d use_ws=%d ws_slice=%lld "
                        "finish_blocks=%u ws_need=%lld",
                        pl.grid, 64 * pl.tm, 64 * pl.tn, pl.splits, pl.rows_per_split, pl.max_wraps, pl.sp_min_steps, (int)pl.use_ws, pl.ws_slice,
                        pl.finish_blocks, pl.ws_need);
  return pp_plan_append(buf, cap, at, "\n");
}
// the merged stride-2 data gradient: f, pl = facts and plan of its heaviest class (the tile every class runs on)
inline int pp_plan_print(char* buf, int cap, int at, const PpIgemmFacts& f, const PpIgemmPlan& pl, const PpS2Merged& g, bool detail) {
  at = pp_plan_append(buf, cap, at, "igemm3 s2 N %d -> tile %dx%d, %d classes:", f.Nout, 64 * pl.tm, 64 * pl.tn, g.n_cls);
  for (int i = 0; i < g.n_cls; ++i)
    at = pp_plan_append(buf, cap, at, " (%d,%d) M %d steps %d", g.c[i].cy, g.c[i].cx, g.c[i].M, g.c[i].kh * g.c[i].kw * (f.Cred / 32));
  at = pp_plan_append(buf, cap, at, " %s", pp_igemm_family_name[PP_IGEMM3F_S2]);
  if (detail) {
    at = pp_plan_append(buf, cap, at, " | grid=%u n_tiles_n=%d class_grids=", g.grid, pl.n_tiles_n);
    for (int i = 0; i < g.n_cls; ++i) at = pp_plan_append(buf, cap, at, i ? "+%d" : "%d", g.c[i].tiles);
  }
  return pp_plan_append(buf, cap, at, "\n");
}
template <class Facts, class Plan>
inline void pp_plan_debug(const Facts& f, const Plan& pl) {
  if (!pp_sw_debug()) return;
  char line[512];
  pp_plan_print(line, (int)sizeof(line), 0, f, pl, false);
  fputs(line, stderr);
}
inline void pp_plan_debug(const PpIgemmFacts& f, const PpIgemmPlan& pl, const PpS2Merged& g) {
  if (!pp_sw_debug()) return;
  char line[512];
  pp_plan_print(line, (int)sizeof(line), 0, f, pl, g, false);
  fputs(line, stderr);
}
