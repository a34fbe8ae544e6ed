// Host-only check of the stride-2 data gradient's class geometry and merged grid (csrc/conv_plan.h: pp_s2_classes, pp_s2_merge)
// against the definition of the convolution.  No GPU, no HIP: build with any C++17 compiler, best with the address and
// undefined-behaviour sanitizers (tests/test_conv_s2_plan_cpu.py does):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I pyrapose_amd/csrc tools/s2_geometry_check.cpp -o s2_check
// Prints one line per case and "ok"; exits 1 at the first violated property.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "conv_plan.h"

#define REQUIRE(cond, ...)                   \
  do {                                       \
    if (!(cond)) {                           \
      fprintf(stderr, "FAILED %s: ", #cond); \
      fprintf(stderr, __VA_ARGS__);          \
      fprintf(stderr, "\n");                 \
      exit(1);                               \
    }                                        \
  } while (0)

// the class a workgroup takes, written as igemm3m_kernel writes it: selects against the prefix sums, no division
static int class_of_workgroup(const PpS2Merged& g, int bid) {
  int ci = 0;
  for (int j = 1; j < 4; ++j)
    if (j < g.n_cls && bid >= g.c[j].blk_begin) ci = j;
  return ci;
}

static void check_case(int n_img, int H, int W, int k, int pad, int Nout) {
  PpS2Class cls[4];
  pp_s2_classes(n_img, H, W, k, k, pad, pad, cls);
  // 1. the classes tile the input grid: every cell in exactly one class, at one position of that class's grid
  std::vector<int> seen((size_t)H * W, 0);
  long long rows = 0;
  for (int c = 0; c < 4; ++c) {
    const PpS2Class& r = cls[c];
    REQUIRE(r.cy == (c >> 1) && r.cx == (c & 1), "class %d", c);
    REQUIRE(r.M == n_img * r.OH * r.OW && r.OH >= 0 && r.OW >= 0, "class %d: M %d", c, r.M);
    REQUIRE((r.kh == 0) == (r.kw == 0), "class %d: taps %d x %d", c, r.kh, r.kw);
    rows += r.M;
    for (int y = 0; y < r.OH; ++y)
      for (int x = 0; x < r.OW; ++x) {
        const int Y = 2 * y + r.cy, X = 2 * x + r.cx;
        REQUIRE(Y < H && X < W, "class %d: cell (%d, %d) outside %d x %d", c, Y, X, H, W);
        seen[(size_t)Y * W + X] += 1;
      }
    // 2. the taps of the class are exactly the taps of the convolution that reach its cells: forward, output cell o reads input
    // cell 2 * o - pad + t, so input cell Y receives tap t from o = (Y + pad - t) / 2 where that is whole
    for (int axis = 0; axis < 2; ++axis) {
      const int par = axis ? r.cx : r.cy, n_t = axis ? r.kw : r.kh, t0 = axis ? r.w_tx0 : r.w_ty0, off = axis ? r.off_x : r.off_y;
      int reach = 0;
      for (int t = 0; t < k; ++t) reach += ((par + pad - t) % 2 == 0) ? 1 : 0;
      if (r.kh > 0) REQUIRE(n_t == reach, "class %d axis %d: %d taps, %d reach it", c, axis, n_t, reach);
      for (int i = 0; i < n_t; ++i) {
        const int t = t0 + 2 * i;  // weight tap of loop tap i (w_tstep = 2)
        REQUIRE(t >= 0 && t < k, "class %d axis %d: weight tap %d", c, axis, t);
        for (int q = 0; q < (axis ? r.OW : r.OH); ++q) {
          const int o = q + off - i;  // gathered cell of class cell q at loop tap i (tsign = -1)
          REQUIRE(2 * o - pad + t == 2 * q + par, "class %d axis %d: cell %d tap %d gathers output cell %d", c, axis, q, i, o);
        }
      }
    }
  }
  REQUIRE(rows == (long long)n_img * H * W, "rows %lld of %d", rows, n_img * H * W);
  for (size_t i = 0; i < seen.size(); ++i) REQUIRE(seen[i] == 1, "cell %zu in %d classes", i, seen[i]);
  // a class without taps exists only where NO tap of the kernel reaches its parity on one axis
  for (int c = 0; c < 4; ++c)
    if (cls[c].kh == 0) {
      int ry = 0, rx = 0;
      for (int t = 0; t < k; ++t) {
        ry += ((cls[c].cy + pad - t) % 2 == 0) ? 1 : 0;
        rx += ((cls[c].cx + pad - t) % 2 == 0) ? 1 : 0;
      }
      REQUIRE(ry == 0 || rx == 0, "class %d lost its taps", c);
    }
  // 3. the merged grid on every tile of the launch functions
  static const int tiles[5][2] = {{256, 128}, {128, 128}, {64, 128}, {128, 64}, {64, 64}};
  for (int ti = 0; ti < 5; ++ti) {
    const int BM = tiles[ti][0], BN = tiles[ti][1];
    const PpS2Merged g = pp_s2_merge(cls, BM, BN, Nout);
    int with_rows = 0;
    for (int c = 0; c < 4; ++c) with_rows += cls[c].M > 0 ? 1 : 0;
    REQUIRE(g.n_cls == with_rows && g.n_cls >= 1, "%d classes in the grid, %d have rows", g.n_cls, with_rows);
    long long at = 0;
    unsigned used = 0;
    for (int i = 0; i < g.n_cls; ++i) {
      const PpS2Class& r = g.c[i];
      const PpS2Class& src = cls[2 * r.cy + r.cx];
      REQUIRE(r.M == src.M && r.M > 0 && r.kh == src.kh && r.kw == src.kw && r.off_y == src.off_y && r.off_x == src.off_x && r.w_ty0 == src.w_ty0 &&
                  r.w_tx0 == src.w_tx0 && r.OH == src.OH && r.OW == src.OW,
              "class %d of the grid is not class (%d, %d)", i, r.cy, r.cx);
      REQUIRE(!(used & (1u << (2 * r.cy + r.cx))), "class (%d, %d) twice", r.cy, r.cx);
      used |= 1u << (2 * r.cy + r.cx);
      if (i > 0) {
        const int t_prev = g.c[i - 1].kh * g.c[i - 1].kw, t = r.kh * r.kw;
        REQUIRE(t_prev > t || (t_prev == t && 2 * g.c[i - 1].cy + g.c[i - 1].cx < 2 * r.cy + r.cx), "order at %d", i);
      }
      REQUIRE(r.tiles == ((r.M + BM - 1) / BM) * ((Nout + BN - 1) / BN) && r.tiles > 0, "tiles of class %d: %d", i, r.tiles);
      REQUIRE(r.blk_begin == at, "prefix sum of class %d: %d, want %lld", i, r.blk_begin, at);
      at += r.tiles;
    }
    REQUIRE(g.grid == (unsigned)at && at < (1ll << 31), "grid %u, classes hold %lld", g.grid, at);
    // every workgroup finds the class whose range holds it, and its index inside the class is a tile of that class
    for (unsigned b = 0; b < g.grid; ++b) {
      const int ci = class_of_workgroup(g, (int)b);
      const int local = (int)b - g.c[ci].blk_begin;
      REQUIRE(local >= 0 && local < g.c[ci].tiles, "workgroup %u -> class %d, tile %d of %d", b, ci, local, g.c[ci].tiles);
    }
  }
  printf("n_img %d  %d x %d  k %d pad %d  N %d: classes M %d %d %d %d, taps %dx%d %dx%d %dx%d %dx%d\n", n_img, H, W, k, pad, Nout, cls[0].M, cls[1].M,
         cls[2].M, cls[3].M, cls[0].kh, cls[0].kw, cls[1].kh, cls[1].kw, cls[2].kh, cls[2].kw, cls[3].kh, cls[3].kw);
}

int main() {
  static const int grids[][3] = {{2, 5, 7},  {2, 6, 5},   {2, 1, 9},   {1, 1, 1},   {3, 9, 1},   {1, 16, 16}, {2, 16, 17},
                                 {1, 17, 30}, {8, 30, 40}, {8, 60, 80}, {1, 33, 31}, {4, 128, 2}, {1, 2, 2}};
  static const int kernels[][2] = {{1, 0}, {3, 0}, {3, 1}, {2, 0}, {2, 1}, {5, 2}, {7, 3}};
  static const int couts[] = {64, 144, 1024};
  for (const auto& gr : grids)
    for (const auto& kp : kernels)
      for (const int n : couts) check_case(gr[0], gr[1], gr[2], kp[0], kp[1], n);
  printf("ok\n");
  return 0;
}
