// Mesh geometry under the renderer, the metrics and the model tools: per-face normals and areas with the mesh's area, signed
// volume and centroid; area-weighted vertex normals with the vertex-to-face adjacency; points drawn uniformly by area from the
// surface.  float64.  Nothing in the reference computes any of this (it reads normals and points from BOP's files): the rules
// are this project's own, restated in tests/mesh_np.py, which every output is bit-identical to ("restated, unpinned").
//   cross product      n = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx), u = p1 - p0, v = p2 - p0
//   squared length     (x x + y y) + z z, a dot product (x x' + y y') + z z'      -- as model_info.hip associates d2
//   sums over faces    chunks of MESH_THREADS faces in face order, each by the halving tree of tile_sum256 (a tail lane adds
//                      +0.0), then the chunks in order by one lane: one fixed order
//   vertex normals     the incident faces' normals added one by one in ascending face index, then divided by the length
//   face of a sample   integers only: areas quantised against the exact maximum, an integer scan, a 64 x 64 -> high 64 multiply
// Compiled with -ffp-contract=off: every product and sum is rounded on its own.  No float atomics; the integer atomics (valence
// counts, fill cursors) never decide a result: the adjacency is put in order by rank afterwards.  No entry point synchronises
// with the host, no workgroup waits on another, every loop is bounded by a count derived from the sizes.  Inputs must be finite.
#include "pose_common.h"
#include "splitmix.h"

#define MESH_THREADS 256          // workgroup size of every kernel here = faces per chunk of the float sums
#define MESH_SCAN_CHUNK 1024      // quantised areas per workgroup of the integer scan: 4 per thread
#define MESH_MAX_ELEMS (1 << 22)  // n_v and n_f at most
#define MESH_MAX_SAMPLES (1 << 24)
#define MESH_MAX_ATTR 8
#define MESH_Q_BITS 39            // the largest quantised area lies in [2^39, 2^40): 2^22 of them stay below 2^62
#define MESH_SEARCH_STEPS 23      // halvings that take 2^22 candidates to one, and one to spare
#define MESH_PARTIAL 8            // doubles per chunk: five sums, the largest area2, the bad-index flag, one spare
#define MESH_WEYL 0x9E3779B97F4A7C15ull

static_assert(MESH_THREADS == POSE_TILE, "tile_sum256 / tile_max256 fold POSE_TILE lanes");
static_assert(MESH_SCAN_CHUNK == 4 * MESH_THREADS, "mesh_scan_tile holds four values per thread");

typedef unsigned long long mesh_u64;

static inline int mesh_chunks(int n, int per) { return (n + per - 1) / per; }
static inline bool mesh_sizes_ok(int n_v, int n_f) { return n_v >= 1 && n_v <= MESH_MAX_ELEMS && n_f >= 1 && n_f <= MESH_MAX_ELEMS; }

// the three vertex indices of face f; false when one of them names no vertex (the face then counts as degenerate everywhere)
__device__ __forceinline__ bool mesh_face(const int* __restrict__ faces, int f, int n_v, int (&idx)[3]) {
  idx[0] = faces[3 * (size_t)f];
  idx[1] = faces[3 * (size_t)f + 1];
  idx[2] = faces[3 * (size_t)f + 2];
  return (unsigned)idx[0] < (unsigned)n_v && (unsigned)idx[1] < (unsigned)n_v && (unsigned)idx[2] < (unsigned)n_v;
}

// ---- 1. face geometry -----------------------------------------------------------------------------------------------------
// One face per thread, one chunk per workgroup.  partial[chunk] = {sum area2, sum p0 . n, sum area2 (p0 + p1 + p2) [3],
// max area2, 1.0 if a face of the chunk names a vertex out of range, 0}.  A face past n_f and a face with a bad index hold three
// zero points: they add +0.0 to every sum and never read pts.

__global__ void __launch_bounds__(MESH_THREADS)
mesh_face_kernel(int n_v, int n_f, const double* __restrict__ pts, const int* __restrict__ faces, double* __restrict__ normal,
                 double* __restrict__ area2, double* __restrict__ partial) {
  __shared__ double red[MESH_THREADS];
  const int tid = threadIdx.x, f = blockIdx.x * MESH_THREADS + tid;
  double p[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  double bad = 0.0;
  if (f < n_f) {
    int idx[3];
    if (mesh_face(faces, f, n_v, idx)) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        p[k][0] = pts[3 * (size_t)idx[k]];
        p[k][1] = pts[3 * (size_t)idx[k] + 1];
        p[k][2] = pts[3 * (size_t)idx[k] + 2];
      }
    } else {
      bad = 1.0;
    }
  }
  const double ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
  const double vx = p[2][0] - p[0][0], vy = p[2][1] - p[0][1], vz = p[2][2] - p[0][2];
  const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  const double a2 = __dsqrt_rn((nx * nx + ny * ny) + nz * nz);
  if (f < n_f) {
    normal[3 * (size_t)f] = nx;
    normal[3 * (size_t)f + 1] = ny;
    normal[3 * (size_t)f + 2] = nz;
    area2[f] = a2;
  }
  double s[5];
  s[0] = a2;
  s[1] = (p[0][0] * nx + p[0][1] * ny) + p[0][2] * nz;
#pragma unroll
  for (int a = 0; a < 3; ++a) s[2 + a] = a2 * ((p[0][a] + p[1][a]) + p[2][a]);
#pragma unroll
  for (int k = 0; k < 5; ++k) s[k] = tile_sum256(s[k], red);
  double m[2] = {a2, bad};
  tile_max256(m, red);
  if (tid == 0) {
    double* out = partial + (size_t)MESH_PARTIAL * blockIdx.x;
#pragma unroll
    for (int k = 0; k < 5; ++k) out[k] = s[k];
    out[5] = m[0];
    out[6] = m[1];
    out[7] = 0.0;
  }
}

// one workgroup: lanes 0..4 add their sum's partials chunk by chunk; all lanes fold the maxima (exact in any order)
__global__ void __launch_bounds__(MESH_THREADS)
mesh_face_finish_kernel(int chunks, const double* __restrict__ partial, double* __restrict__ totals, int* __restrict__ status) {
  __shared__ double red[2 * (MESH_THREADS / 64)];
  const int tid = threadIdx.x;
  if (tid < 5) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += partial[(size_t)MESH_PARTIAL * c + tid];
    totals[tid] = s;
  }
  double m[2] = {0.0, 0.0};
  for (int c = tid; c < chunks; c += MESH_THREADS) {
    const double a = partial[(size_t)MESH_PARTIAL * c + 5], b = partial[(size_t)MESH_PARTIAL * c + 6];
    m[0] = a > m[0] ? a : m[0];
    m[1] = b > m[1] ? b : m[1];
  }
  tile_max256(m, red);
  if (tid == 0) {
    totals[5] = m[0];
    totals[6] = 0.0;
    totals[7] = 0.0;
    status[0] = (m[1] > 0.0 ? 1 : 0) | (m[0] > 0.0 ? 0 : 2);
  }
}

extern "C" size_t pp_mesh_face_geometry_workspace_bytes(int n_f) {
  if (n_f <= 0 || n_f > MESH_MAX_ELEMS) return 0;
  return (size_t)mesh_chunks(n_f, MESH_THREADS) * MESH_PARTIAL * sizeof(double);
}

extern "C" int pp_mesh_face_geometry_f64(pp_ctx* ctx, int n_v, int n_f, const double* pts, const int* faces, void* workspace,
                                         size_t workspace_bytes, double* normal, double* area2, double* totals, int* status) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, mesh_sizes_ok(n_v, n_f), PP_ERR_SHAPE, "pp_mesh_face_geometry_f64: need 1..%d vertices and faces, got %d and %d",
               MESH_MAX_ELEMS, n_v, n_f);
  PP_CHECK_ARG(ctx, pts && faces && workspace && normal && area2 && totals && status, PP_ERR_ARG, "pp_mesh_face_geometry_f64: null argument");
  PP_CHECK_ARG(ctx, workspace_bytes >= pp_mesh_face_geometry_workspace_bytes(n_f), PP_ERR_ARG,
               "pp_mesh_face_geometry_f64: workspace of %zu bytes, need %zu (pp_mesh_face_geometry_workspace_bytes)", workspace_bytes,
               pp_mesh_face_geometry_workspace_bytes(n_f));
  const int chunks = mesh_chunks(n_f, MESH_THREADS);
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(mesh_face_kernel, dim3(chunks), dim3(MESH_THREADS), 0, ctx->stream, n_v, n_f, pts, faces, normal, area2, partial);
  hipLaunchKernelGGL(mesh_face_finish_kernel, dim3(1), dim3(MESH_THREADS), 0, ctx->stream, chunks, (const double*)partial, totals, status);
  PP_CHECK_LAUNCH(ctx, "pp_mesh_face_geometry_f64");
  return PP_OK;
}

// ---- 2. vertex normals and the vertex-to-face adjacency ---------------------------------------------------------------------
// An incidence is e = 3 f + k: vertex k of face f, of a face whose three indices are all in range.  count: valence per vertex
// (integer atomics) -> the existing one-workgroup exclusive scan: adj_offsets and the fill cursors -> fill: every incidence
// takes a slot of its vertex's segment in whatever order the atomics land -> rank: the thread of a slot counts the segment's
// smaller incidences and writes its face at that rank.  Incidences are distinct, so the ranks are a permutation and the segment
// comes out ascending whatever the fill order was.  A hub of valence V costs V lanes V steps each, spread over the grid, not one
// lane V^2; the sum over a vertex's segment is one lane's V additions, as the ascending order of the rule demands.

__global__ void __launch_bounds__(MESH_THREADS)
mesh_valence_kernel(int n_v, int n_f, const int* __restrict__ faces, int* __restrict__ counts) {
  const int f = blockIdx.x * MESH_THREADS + threadIdx.x;
  int idx[3];
  if (f >= n_f || !mesh_face(faces, f, n_v, idx)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) atomicAdd(&counts[idx[k]], 1);
}

__global__ void __launch_bounds__(MESH_THREADS)
mesh_fill_kernel(int n_v, int n_f, const int* __restrict__ faces, int* __restrict__ cursor, int* __restrict__ slots) {
  const int f = blockIdx.x * MESH_THREADS + threadIdx.x;
  int idx[3];
  if (f >= n_f || !mesh_face(faces, f, n_v, idx)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int at = atomicAdd(&cursor[idx[k]], 1);
    if ((unsigned)at < 3u * (unsigned)n_f) slots[at] = 3 * f + k;  // (always: the cursors start at the offsets of these same counts)
  }
}

__global__ void __launch_bounds__(MESH_THREADS)
mesh_rank_kernel(int n_v, int n_f, const int* __restrict__ faces, const int* __restrict__ offsets, const int* __restrict__ slots,
                 int* __restrict__ adj_faces) {
  const int at = blockIdx.x * MESH_THREADS + threadIdx.x;
  if (at >= 3 * n_f) return;
  if (at >= offsets[n_v]) {  // past the last segment: the incidences of faces with a bad index are not listed
    adj_faces[at] = -1;
    return;
  }
  const int e = slots[at], v = faces[e];
  const int begin = offsets[v], len = min(offsets[v + 1] - begin, 3 * n_f);
  int rank = 0;
  for (int j = 0; j < len; ++j) rank += slots[begin + j] < e ? 1 : 0;
  adj_faces[begin + rank] = e / 3;
}

__global__ void __launch_bounds__(MESH_THREADS)
mesh_vertex_normal_kernel(int n_v, int n_f, const double* __restrict__ face_normal, const double* __restrict__ totals, int outward,
                          const int* __restrict__ offsets, const int* __restrict__ adj_faces, double* __restrict__ vnormal) {
  const int v = blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= n_v) return;
  const bool flip = outward != 0 && totals[1] < 0.0;
  const int begin = offsets[v], len = min(offsets[v + 1] - begin, 3 * n_f);
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int j = 0; j < len; ++j) {
    const size_t f = (size_t)min(max(adj_faces[begin + j], 0), n_f - 1);  // (in range already: the ranks are a permutation)
    sx += face_normal[3 * f];
    sy += face_normal[3 * f + 1];
    sz += face_normal[3 * f + 2];
  }
  const double l = __dsqrt_rn((sx * sx + sy * sy) + sz * sz);
  double ox = 0.0, oy = 0.0, oz = 0.0;
  if (l > 0.0) {
    ox = sx / l;
    oy = sy / l;
    oz = sz / l;
    if (flip) {
      ox = -ox;
      oy = -oy;
      oz = -oz;
    }
  }
  vnormal[3 * (size_t)v] = ox;
  vnormal[3 * (size_t)v + 1] = oy;
  vnormal[3 * (size_t)v + 2] = oz;
}

// workspace: counts [n_v] | cursor [n_v] | slots [3 n_f], each from a 256-byte boundary
extern "C" size_t pp_mesh_vertex_normals_workspace_bytes(int n_v, int n_f) {
  if (!mesh_sizes_ok(n_v, n_f)) return 0;
  return 2 * pp_align256((size_t)n_v * sizeof(int)) + 3 * (size_t)n_f * sizeof(int);
}

extern "C" int pp_mesh_vertex_normals_f64(pp_ctx* ctx, int n_v, int n_f, const int* faces, const double* face_normal, const double* totals,
                                          int outward, void* workspace, size_t workspace_bytes, double* vnormal, int* adj_offsets,
                                          int* adj_faces) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, mesh_sizes_ok(n_v, n_f), PP_ERR_SHAPE, "pp_mesh_vertex_normals_f64: need 1..%d vertices and faces, got %d and %d",
               MESH_MAX_ELEMS, n_v, n_f);
  PP_CHECK_ARG(ctx, faces && face_normal && totals && workspace && vnormal && adj_offsets && adj_faces, PP_ERR_ARG,
               "pp_mesh_vertex_normals_f64: null argument");
  PP_CHECK_ARG(ctx, workspace_bytes >= pp_mesh_vertex_normals_workspace_bytes(n_v, n_f), PP_ERR_ARG,
               "pp_mesh_vertex_normals_f64: workspace of %zu bytes, need %zu (pp_mesh_vertex_normals_workspace_bytes)", workspace_bytes,
               pp_mesh_vertex_normals_workspace_bytes(n_v, n_f));
  int* counts = (int*)workspace;
  int* cursor = (int*)((char*)workspace + pp_align256((size_t)n_v * sizeof(int)));
  int* slots = (int*)((char*)workspace + 2 * pp_align256((size_t)n_v * sizeof(int)));
  const int face_groups = mesh_chunks(n_f, MESH_THREADS);
  PP_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)n_v * sizeof(int), ctx->stream));
  hipLaunchKernelGGL(mesh_valence_kernel, dim3(face_groups), dim3(MESH_THREADS), 0, ctx->stream, n_v, n_f, faces, counts);
  hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, n_v, (const int*)counts, adj_offsets, cursor);
  hipLaunchKernelGGL(mesh_fill_kernel, dim3(face_groups), dim3(MESH_THREADS), 0, ctx->stream, n_v, n_f, faces, cursor, slots);
  hipLaunchKernelGGL(mesh_rank_kernel, dim3(mesh_chunks(3 * n_f, MESH_THREADS)), dim3(MESH_THREADS), 0, ctx->stream, n_v, n_f, faces,
                     (const int*)adj_offsets, (const int*)slots, adj_faces);
  hipLaunchKernelGGL(mesh_vertex_normal_kernel, dim3(mesh_chunks(n_v, MESH_THREADS)), dim3(MESH_THREADS), 0, ctx->stream, n_v, n_f,
                     face_normal, totals, outward, (const int*)adj_offsets, (const int*)adj_faces, vnormal);
  PP_CHECK_LAUNCH(ctx, "pp_mesh_vertex_normals_f64");
  return PP_OK;
}

// ---- 3. surface samples ---------------------------------------------------------------------------------------------------
// quantise: q_f = floor(ldexp(area2_f, 39 - ilogb(max area2))), 0 for a face with a bad index; each workgroup leaves the
// inclusive sums within its chunk of MESH_SCAN_CHUNK in cum[] and the chunk's total in ctot[] -> one workgroup turns ctot[] into
// the chunks' exclusive bases and ctot[chunks] into the grand total -> every chunk adds its base: cum[f] = q_0 + ... + q_f.
// Integer sums are exact: the shape of the scan does not show in the result.  sample i then draws
//   word(j) = splitmix64(splitmix64(4 seed + j) + i)            j = 0 the face, 1 and 2 the barycentrics
//   u = word(0), or in mode 1 the Weyl sequence splitmix64(4 seed + 3) + i 0x9E3779B97F4A7C15 (mod 2^64)
//   face = the first f with cum[f] > hi64(u * total)             a face with q_f = 0 is never the first: never chosen
//   r1, r2 = (word(1) >> 11) 2^-53, (word(2) >> 11) 2^-53;  s = sqrt(r1);  a = 1 - s, b = s (1 - r2), c = s r2
//   point = (a p0 + b p1) + c p2 per coordinate, attributes alike; normal = the face's normal / area2, negated for an inward mesh

// the inclusive sums of the workgroup's 4 * MESH_THREADS values, four consecutive ones per thread, in place; returns their total
__device__ __forceinline__ mesh_u64 mesh_scan_tile(mesh_u64 (&v)[4], mesh_u64* s) {
  const int tid = threadIdx.x;
  v[1] += v[0];
  v[2] += v[1];
  v[3] += v[2];
  s[tid] = v[3];
  __syncthreads();
  for (int off = 1; off < MESH_THREADS; off <<= 1) {
    const mesh_u64 u = tid >= off ? s[tid - off] : 0ull;
    __syncthreads();
    s[tid] += u;
    __syncthreads();
  }
  const mesh_u64 before = s[tid] - v[3], total = s[MESH_THREADS - 1];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] += before;
  return total;
}

__global__ void __launch_bounds__(MESH_THREADS)
mesh_quantise_kernel(int n_v, int n_f, const int* __restrict__ faces, const double* __restrict__ area2, const double* __restrict__ totals,
                     mesh_u64* __restrict__ cum, mesh_u64* __restrict__ ctot) {
  __shared__ mesh_u64 s[MESH_THREADS];
  const double largest = totals[5];
  const bool any = largest > 0.0;
  const int shift = any ? MESH_Q_BITS - ilogb(largest) : 0;
  const int f0 = blockIdx.x * MESH_SCAN_CHUNK + 4 * threadIdx.x;
  mesh_u64 v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int f = f0 + k;
    int idx[3];
    v[k] = 0ull;
    if (any && f < n_f && mesh_face(faces, f, n_v, idx)) {
      const double a = area2[f];
      if (a > 0.0 && a <= largest) v[k] = (mesh_u64)floor(ldexp(a, shift));  // (an area outside (0, max] is not one step 1 wrote)
    }
  }
  const mesh_u64 total = mesh_scan_tile(v, s);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (f0 + k < n_f) cum[f0 + k] = v[k];
  if (threadIdx.x == 0) ctot[blockIdx.x] = total;
}

// one workgroup: ctot[0..chunks) -> the exclusive sums, ctot[chunks] = the total
__global__ void __launch_bounds__(MESH_THREADS)
mesh_scan_totals_kernel(int chunks, mesh_u64* __restrict__ ctot) {
  __shared__ mesh_u64 s[MESH_THREADS];
  mesh_u64 carry = 0ull;
  for (int base = 0; base < chunks; base += MESH_SCAN_CHUNK) {
    const int c0 = base + 4 * threadIdx.x;
    mesh_u64 v[4], own[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) own[k] = v[k] = c0 + k < chunks ? ctot[c0 + k] : 0ull;
    const mesh_u64 total = mesh_scan_tile(v, s);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c0 + k < chunks) ctot[c0 + k] = carry + (v[k] - own[k]);
    carry += total;
  }
  if (threadIdx.x == 0) ctot[chunks] = carry;
}

__global__ void __launch_bounds__(MESH_THREADS)
mesh_add_base_kernel(int n_f, const mesh_u64* __restrict__ ctot, mesh_u64* __restrict__ cum) {
  const int f = blockIdx.x * MESH_THREADS + threadIdx.x;
  if (f < n_f) cum[f] += ctot[f / MESH_SCAN_CHUNK];
}

__global__ void __launch_bounds__(MESH_THREADS)
mesh_sample_kernel(int n_v, int n_f, int chunks, const double* __restrict__ pts, const int* __restrict__ faces,
                   const double* __restrict__ face_normal, const double* __restrict__ area2, const double* __restrict__ totals,
                   const mesh_u64* __restrict__ cum, const mesh_u64* __restrict__ ctot, int n_samples, mesh_u64 seed, int mode,
                   int outward, int n_attr, const double* __restrict__ attr, double* __restrict__ points, int* __restrict__ face,
                   double* __restrict__ bary, double* __restrict__ normals, double* __restrict__ attr_out) {
  const int i = blockIdx.x * MESH_THREADS + threadIdx.x;
  if (i >= n_samples) return;
  const mesh_u64 total = ctot[chunks];
  int f = -1, idx[3] = {0, 0, 0};
  double w[3] = {0.0, 0.0, 0.0};
  if (total > 0ull) {
    const mesh_u64 u = mode == 0 ? splitmix64(splitmix64(4ull * seed) + (mesh_u64)i) : splitmix64(4ull * seed + 3ull) + (mesh_u64)i * MESH_WEYL;
    const mesh_u64 t = __umul64hi(u, total);
    int lo = 0, hi = n_f - 1;
    for (int step = 0; step < MESH_SEARCH_STEPS && lo < hi; ++step) {
      const int mid = (lo + hi) >> 1;
      if (cum[mid] > t)
        hi = mid;
      else
        lo = mid + 1;
    }
    if (mesh_face(faces, lo, n_v, idx)) {  // (always: a face with a bad index has q = 0)
      f = lo;
      const double r1 = (double)(splitmix64(splitmix64(4ull * seed + 1ull) + (mesh_u64)i) >> 11) * 0x1p-53;
      const double r2 = (double)(splitmix64(splitmix64(4ull * seed + 2ull) + (mesh_u64)i) >> 11) * 0x1p-53;
      const double s = __dsqrt_rn(r1);
      w[0] = 1.0 - s;
      w[1] = s * (1.0 - r2);
      w[2] = s * r2;
    }
  }
  const bool have = f >= 0;
  if (face) face[i] = f;
  if (bary) {
#pragma unroll
    for (int k = 0; k < 3; ++k) bary[3 * (size_t)i + k] = w[k];
  }
  if (points) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double r = 0.0;
      if (have) r = (w[0] * pts[3 * (size_t)idx[0] + a] + w[1] * pts[3 * (size_t)idx[1] + a]) + w[2] * pts[3 * (size_t)idx[2] + a];
      points[3 * (size_t)i + a] = r;
    }
  }
  if (normals) {
    const bool flip = outward != 0 && totals[1] < 0.0;
    const double l = have ? area2[f] : 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double r = 0.0;
      if (have && l > 0.0) {
        r = face_normal[3 * (size_t)f + a] / l;
        r = flip ? -r : r;
      }
      normals[3 * (size_t)i + a] = r;
    }
  }
  if (attr_out) {
    for (int a = 0; a < n_attr; ++a) {
      double r = 0.0;
      if (have)
        r = (w[0] * attr[(size_t)n_attr * idx[0] + a] + w[1] * attr[(size_t)n_attr * idx[1] + a]) + w[2] * attr[(size_t)n_attr * idx[2] + a];
      attr_out[(size_t)n_attr * i + a] = r;
    }
  }
}

// workspace: cum [n_f] | ctot [chunks + 1]
extern "C" size_t pp_mesh_sample_surface_workspace_bytes(int n_f) {
  if (n_f <= 0 || n_f > MESH_MAX_ELEMS) return 0;
  return pp_align256((size_t)n_f * sizeof(mesh_u64)) + ((size_t)mesh_chunks(n_f, MESH_SCAN_CHUNK) + 1) * sizeof(mesh_u64);
}

extern "C" int pp_mesh_sample_surface_f64(pp_ctx* ctx, int n_v, int n_f, const double* pts, const int* faces, const double* face_normal,
                                          const double* area2, const double* totals, int n_samples, unsigned long long seed, int mode,
                                          int outward, int n_attr, const double* attr, void* workspace, size_t workspace_bytes,
                                          double* points, int* face, double* bary, double* normals, double* attr_out) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, mesh_sizes_ok(n_v, n_f), PP_ERR_SHAPE, "pp_mesh_sample_surface_f64: need 1..%d vertices and faces, got %d and %d",
               MESH_MAX_ELEMS, n_v, n_f);
  PP_CHECK_ARG(ctx, n_samples >= 1 && n_samples <= MESH_MAX_SAMPLES, PP_ERR_SHAPE, "pp_mesh_sample_surface_f64: need 1..%d samples, got %d",
               MESH_MAX_SAMPLES, n_samples);
  PP_CHECK_ARG(ctx, !attr_out || (n_attr >= 1 && n_attr <= MESH_MAX_ATTR), PP_ERR_SHAPE,
               "pp_mesh_sample_surface_f64: need 1..%d attributes per vertex, got %d", MESH_MAX_ATTR, n_attr);
  PP_CHECK_ARG(ctx, mode == 0 || mode == 1, PP_ERR_ARG, "pp_mesh_sample_surface_f64: mode must be 0 (random) or 1 (Weyl), got %d", mode);
  PP_CHECK_ARG(ctx, pts && faces && face_normal && area2 && totals && workspace && (attr || !attr_out), PP_ERR_ARG,
               "pp_mesh_sample_surface_f64: null argument");
  PP_CHECK_ARG(ctx, workspace_bytes >= pp_mesh_sample_surface_workspace_bytes(n_f), PP_ERR_ARG,
               "pp_mesh_sample_surface_f64: workspace of %zu bytes, need %zu (pp_mesh_sample_surface_workspace_bytes)", workspace_bytes,
               pp_mesh_sample_surface_workspace_bytes(n_f));
  const int chunks = mesh_chunks(n_f, MESH_SCAN_CHUNK);
  mesh_u64* cum = (mesh_u64*)workspace;
  mesh_u64* ctot = (mesh_u64*)((char*)workspace + pp_align256((size_t)n_f * sizeof(mesh_u64)));
  hipLaunchKernelGGL(mesh_quantise_kernel, dim3(chunks), dim3(MESH_THREADS), 0, ctx->stream, n_v, n_f, faces, area2, totals, cum, ctot);
  hipLaunchKernelGGL(mesh_scan_totals_kernel, dim3(1), dim3(MESH_THREADS), 0, ctx->stream, chunks, ctot);
  hipLaunchKernelGGL(mesh_add_base_kernel, dim3(mesh_chunks(n_f, MESH_THREADS)), dim3(MESH_THREADS), 0, ctx->stream, n_f,
                     (const mesh_u64*)ctot, cum);
  hipLaunchKernelGGL(mesh_sample_kernel, dim3(mesh_chunks(n_samples, MESH_THREADS)), dim3(MESH_THREADS), 0, ctx->stream, n_v, n_f, chunks, pts,
                     faces, face_normal, area2, totals, (const mesh_u64*)cum, (const mesh_u64*)ctot, n_samples, (mesh_u64)seed, mode, outward,
                     attr_out ? n_attr : 0, attr, points, face, bary, normals, attr_out);
  PP_CHECK_LAUNCH(ctx, "pp_mesh_sample_surface_f64");
  return PP_OK;
}
