// The raster phase of the workgroup of (pose, tile), included into the body of each of the three raster kernels (render.hip's
// depth kernel, render_rgbd_raster.inc's two): the z-buffer zb [RT * RT] set to RASTER_EMPTY, then the tile's list and the pose's
// big list in chunks of RASTER_THREADS -- a thread rasterises its small triangle itself, larger ones go through queue
// [RASTER_THREADS] / qn to the whole workgroup.  Afterwards zb is resolved and every thread may read it.  The includer defines
// RASTER_EMPTY and has in scope zb, queue, qn (LDS), pose, tile, tid, r0, c0, vtx and the kernel's parameters.  A text and not
// a function: inlined from a function the same statements compile to other instructions (DESIGN.md), from here to the parent's.
  for (int k = tid; k < RT * RT; k += RASTER_THREADS) zb[k] = RASTER_EMPTY;
  if (tid == 0) qn = 0;
  __syncthreads();
  const size_t b = (size_t)pose * n_tiles + tile;
  const int l0 = offsets[b], l1 = offsets[b + 1];
  for (int base = l0; base < l1; base += RASTER_THREADS) {
    if (base + tid < l1) {
      const int tri = list[base + tid];
      tri_setup T;
      if (setup_triangle(vtx, n_vert, faces, tri, width, height, &T)) {
        const int a0 = max(T.c0, c0), a1 = min(T.c1, c0 + RT - 1), b0 = max(T.r0, r0), b1 = min(T.r1, r0 + RT - 1);
        const int area = (a1 - a0 + 1) * (b1 - b0 + 1);
        if (a0 <= a1 && b0 <= b1) {
          if (area <= RASTER_SMALL_PX) {
            for (int r = b0; r <= b1; ++r)
              for (int c = a0; c <= a1; ++c) raster_px(zb, T, tri, r, c, r0, c0, zn, zf);
          } else {
            queue[atomicAdd(&qn, 1)] = tri;
          }
        }
      }
    }
    __syncthreads();
    raster_queue(zb, queue, qn, vtx, n_vert, faces, width, height, r0, c0, zn, zf);
    __syncthreads();
    if (tid == 0) qn = 0;
    __syncthreads();
  }
  const int nb = big_n[pose];
  for (int base = 0; base < nb; base += RASTER_THREADS) {
    if (base + tid < nb) {
      const int tri = big[(size_t)pose * n_tri + base + tid];
      tri_setup T;
      if (setup_triangle(vtx, n_vert, faces, tri, width, height, &T) && T.c0 < c0 + RT && T.c1 >= c0 && T.r0 < r0 + RT && T.r1 >= r0)
        queue[atomicAdd(&qn, 1)] = tri;
    }
    __syncthreads();
    raster_queue(zb, queue, qn, vtx, n_vert, faces, width, height, r0, c0, zn, zf);
    __syncthreads();
    if (tid == 0) qn = 0;
    __syncthreads();
  }
#undef RASTER_EMPTY
