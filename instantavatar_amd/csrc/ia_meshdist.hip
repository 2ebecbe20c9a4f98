// ia_meshdist.hip -- distance from points to a triangle mesh (no counterpart in the reference): a uniform grid of triangles, the
// closest point of the mesh for many query points, deterministic surface samples.
//   the number of (face, cell) pairs                                                              (ia_meshdist_grid_count)
//   per face a record of its corners, per cell the offset and the list of its faces               (ia_meshdist_grid_build)
//   one lane per query point: shells of cells around the point's cell until the bound ends it     (ia_meshdist_closest)
//   stratified samples over the area with the R2 sequence inside the face                         (ia_meshdist_sample)
// The definitions are stated in DESIGN.md section 4 ("surface distance") and in include/instantavatar_hip_meshdist.h.  Nothing here
// synchronises, allocates or reads on the host.
//
// Why the result does not depend on the grid.  A point's result is the minimum of (d2, face) over every face the walk evaluates, d2
// being one fixed fp64 expression of the point and the face's corners; the walk may only stop when every face it has not evaluated
// has d2 > the best.  A face is listed in the block of cells [cell(min corner), cell(max corner)] per axis, with the fp32 cell
// function of ia_mesh_dev.h (ia_grid_cell), which is monotone in the coordinate.  After shell r the visited cells are the block [c - r, c + r]
// (clamped); a face listed nowhere in it has, on some axis a, cell(min_a) >= c_a + r + 1 or cell(max_a) <= c_a - r - 1.  The fp32
// value t = fl(fl(x - lo) inv_h) differs from (x - lo) / h by a factor within (1 +- 2^-24)^3, so in the first case every coordinate of
// the face is >= lo + (c_a + r + 1)(1 - 2^-22) h and in the second <= lo + (c_a - r)(1 + 2^-22) h: the distance of the point's own
// coordinate to that plane bounds its distance to the face from below, wherever the point and the face lie relative to the box.  The
// smallest such distance over the sides of the block that are not flush with the grid's boundary (negative ones count as 0) bounds
// everything unvisited.  The argument never uses that c is the point's geometric cell, only that the shells are centred on it.
// The grid, its cell function and the face pieces are ia_mesh_dev.h's; the scan of the cells' counts and the fill are ia_scan.h's.
#include "ia_common.h"
#include "ia_mesh_dev.h"
#include "ia_scan.h"
#include "../../include/instantavatar_hip_meshdist.h"

static_assert(IA_MD_THREADS == IA_SCAN_THREADS, "md_carve sizes the block sums for the scan's workgroups");

namespace {

// the corners of face f when it is valid: indices in [0, nv), pairwise different, finite corners, n = (p1 - p0) x (p2 - p0) finite and
// not zero in fp64.  n is returned as well.
__device__ __forceinline__ bool md_face(const float *__restrict__ verts, const int32_t *__restrict__ faces, int f, int nv, float p[3][3],
                                        double n[3]) {
  int v[3];
  ia_face_load(faces, f, v);
  if (!ia_face_in_range(v, nv) || !ia_face_distinct(v)) return false;
  ia_face_corners(verts, v, p);
  if (!ia_corners_finite(p)) return false;
  ia_face_cross(p, n);
  if (!ia_finite3(n[0], n[1], n[2])) return false;
  return n[0] != 0.0 || n[1] != 0.0 || n[2] != 0.0;
}

// (the block of cells of a face, md_range, and the workspace's layout, md_carve, are ia_mesh_dev.h's: ia_meshray.hip reads the same grid)
__global__ __launch_bounds__(IA_MD_THREADS) void k_md_zero64(unsigned long long *p) { if (threadIdx.x == 0 && blockIdx.x == 0) *p = 0ull; }

__global__ __launch_bounds__(IA_MD_THREADS) void k_md_count(const float *__restrict__ verts, const int32_t *__restrict__ faces, int nv, int nf,
                                                            IaGrid G, unsigned long long *total) {
  const long long f = (long long)blockIdx.x * IA_MD_THREADS + threadIdx.x;
  unsigned long long mine = 0ull;
  if (f < nf) {
    float p[3][3];
    double n[3];
    if (md_face(verts, faces, (int)f, nv, p, n)) {
      int c0[3], c1[3];
      md_range(G, p, c0, c1);
      mine = (unsigned long long)(c1[0] - c0[0] + 1) * (unsigned long long)(c1[1] - c0[1] + 1) * (unsigned long long)(c1[2] - c0[2] + 1);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if (ia_lane() == 0 && mine) atomicAdd(total, mine);
}

// pass 0: the face's record (three corners, or NaN for a face that is not valid) and the cells' counts; pass 1: the lists, through a
// cursor per cell.  A slot at or past n_pairs is not written (the caller's count was of another input).
__global__ __launch_bounds__(IA_MD_THREADS) void k_md_emit(const float *__restrict__ verts, const int32_t *__restrict__ faces, int nv, int nf,
                                                           IaGrid G, int pass, float4 *__restrict__ tri, int32_t *cnt,
                                                           const int32_t *__restrict__ start, int32_t *__restrict__ pairs, long long n_pairs) {
  const long long f = (long long)blockIdx.x * IA_MD_THREADS + threadIdx.x;
  if (f >= nf) return;
  float p[3][3];
  double n[3];
  const bool ok = md_face(verts, faces, (int)f, nv, p, n);
  if (pass == 0) {
    const float q = __builtin_nanf("");
    tri[3 * f] = ok ? make_float4(p[0][0], p[0][1], p[0][2], 0.f) : make_float4(q, q, q, q);
    tri[3 * f + 1] = ok ? make_float4(p[1][0], p[1][1], p[1][2], 0.f) : make_float4(q, q, q, q);
    tri[3 * f + 2] = ok ? make_float4(p[2][0], p[2][1], p[2][2], 0.f) : make_float4(q, q, q, q);
  }
  if (!ok) return;
  int c0[3], c1[3];
  md_range(G, p, c0, c1);
  for (int i = c0[0]; i <= c1[0]; i++)
    for (int j = c0[1]; j <= c1[1]; j++)
      for (int k = c0[2]; k <= c1[2]; k++) {
        const long long key = ((long long)i * G.n[1] + j) * G.n[2] + k;
        const int slot = atomicAdd(&cnt[key], 1);
        if (pass == 1) {
          const long long at = (long long)start[key] + slot;
          if (at < n_pairs) pairs[at] = (int32_t)f;
        }
      }
}

// the size, the box and the cell edge, checked; the grid and its number of cells
static_assert(IA_MESHDIST_MAX_CELLS == 16777216ll, "the text below");
int md_check(const char *who, int nf, const float lo[3], const float hi[3], float h, float inv_h, IaGrid *G, long long *cells) {
  IA_CHECK_ARG(nf >= 0, "%s: nf = %d < 0", who, nf);
  IA_CHECK_ARG(nf <= IA_MESHDIST_MAX_FACES, "%s: nf = %d above %d", who, nf, IA_MESHDIST_MAX_FACES);
  return ia_grid_check(who, lo, hi, h, inv_h, true, IA_MESHDIST_MAX_CELLS, "16777216", G, cells);
}

// ---------------------------------------------------------------------------------------------------------------------
// closest point of one triangle (Ericson 5.1.5), fp64, no contraction (the build has -ffp-contract=off)
// ---------------------------------------------------------------------------------------------------------------------
struct MdHit { double d2, u, v, w, c[3]; };

__device__ __forceinline__ void md_point_triangle(const double p[3], const double a[3], const double b[3], const double c[3], MdHit &o) {
  double ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
  for (int d = 0; d < 3; d++) {
    ab[d] = b[d] - a[d]; ac[d] = c[d] - a[d];
    ap[d] = p[d] - a[d]; bp[d] = p[d] - b[d]; cp[d] = p[d] - c[d];
  }
  const double d1 = ia_dot3d(ab, ap), d2 = ia_dot3d(ac, ap);
  const double d3 = ia_dot3d(ab, bp), d4 = ia_dot3d(ac, bp);
  const double d5 = ia_dot3d(ab, cp), d6 = ia_dot3d(ac, cp);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  double u, v, w;
  if (d1 <= 0.0 && d2 <= 0.0) { u = 1.0; v = 0.0; w = 0.0; }                                  // vertex p0
  else if (d3 >= 0.0 && d4 <= d3) { u = 0.0; v = 1.0; w = 0.0; }                              // vertex p1
  else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { v = d1 / (d1 - d3); u = 1.0 - v; w = 0.0; } // edge p0 p1
  else if (d6 >= 0.0 && d5 <= d6) { u = 0.0; v = 0.0; w = 1.0; }                              // vertex p2
  else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { w = d2 / (d2 - d6); u = 1.0 - w; v = 0.0; } // edge p0 p2
  else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {                               // edge p1 p2
    w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); v = 1.0 - w; u = 0.0;
  } else {                                                                                    // the face
    const double den = 1.0 / ((va + vb) + vc);
    v = vb * den; w = vc * den; u = (1.0 - v) - w;
  }
  double s = 0.0;
#pragma unroll
  for (int d = 0; d < 3; d++) {
    o.c[d] = (u * a[d] + v * b[d]) + w * c[d];
    const double e = p[d] - o.c[d];
    s = d == 0 ? e * e : s + e * e;
  }
  o.d2 = s; o.u = u; o.v = v; o.w = w;
}

// (the closest point itself is formed again from the winner's corners at the end, by the same expression: six registers less in the walk)
struct MdBest { double d2, u, v, w; int face; int tests; };

__device__ __forceinline__ void md_visit(long long key, const double p[3], const float4 *__restrict__ tri, const int32_t *__restrict__ start,
                                         const int32_t *__restrict__ pairs, long long n_pairs, int nf, MdBest &B) {
  const int t0 = start[key];
  long long t1 = start[key + 1];
  if (t1 > n_pairs) t1 = n_pairs;
  for (long long t = t0; t < t1; t++) {
    const int f = pairs[t];
    if ((uint32_t)f >= (uint32_t)nf) continue;          // (never for a list that grid_build made)
    const float4 A = tri[3 * (size_t)f], Bc = tri[3 * (size_t)f + 1], C = tri[3 * (size_t)f + 2];
    const double a[3] = {(double)A.x, (double)A.y, (double)A.z}, b[3] = {(double)Bc.x, (double)Bc.y, (double)Bc.z},
                 c[3] = {(double)C.x, (double)C.y, (double)C.z};
    MdHit h;
    md_point_triangle(p, a, b, c, h);
    B.tests++;
    if (h.d2 < B.d2 || (h.d2 == B.d2 && f < B.face)) {
      B.d2 = h.d2; B.u = h.u; B.v = h.v; B.w = h.w; B.face = f;
    }
  }
}

__global__ __launch_bounds__(IA_MD_THREADS) void k_md_closest(const float *__restrict__ points, int P, int nf, IaGrid G, long long n_pairs,
                                                              const float4 *__restrict__ tri, const int32_t *__restrict__ start,
                                                              const int32_t *__restrict__ pairs, float *__restrict__ dist,
                                                              int32_t *__restrict__ face, float *__restrict__ bary, float *__restrict__ closest,
                                                              int32_t *__restrict__ tests) {
  const long long i = (long long)blockIdx.x * IA_MD_THREADS + threadIdx.x;
  if (i >= P) return;
  const float pf[3] = {points[(size_t)i * 3], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2]};
  MdBest B;
  B.d2 = (double)INFINITY; B.u = B.v = B.w = 0.0; B.face = -1; B.tests = 0;
  const bool fin = ia_finite3(pf[0], pf[1], pf[2]);
  if (fin) {
    const double p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
    int c[3];
    int rmax = 0;
#pragma unroll
    for (int d = 0; d < 3; d++) {
      c[d] = ia_grid_cell(pf[d], G.lo[d], G.inv_h, G.n[d]);
      const int far = c[d] > G.n[d] - 1 - c[d] ? c[d] : G.n[d] - 1 - c[d];
      rmax = far > rmax ? far : rmax;
    }
    const double h = (double)G.h, shrink = 1.0 - 0x1p-22, grow = 1.0 + 0x1p-22;
    for (int r = 0; r <= rmax; r++) {
      const int i0 = c[0] - r > 0 ? c[0] - r : 0, i1 = c[0] + r < G.n[0] - 1 ? c[0] + r : G.n[0] - 1;
      const int j0 = c[1] - r > 0 ? c[1] - r : 0, j1 = c[1] + r < G.n[1] - 1 ? c[1] + r : G.n[1] - 1;
      const int k0 = c[2] - r > 0 ? c[2] - r : 0, k1 = c[2] + r < G.n[2] - 1 ? c[2] + r : G.n[2] - 1;
      for (int ii = i0; ii <= i1; ii++) {
        const bool on_i = ii - c[0] == r || c[0] - ii == r;
        for (int jj = j0; jj <= j1; jj++) {
          const long long row = ((long long)ii * G.n[1] + jj) * G.n[2];
          if (on_i || jj - c[1] == r || c[1] - jj == r) {                      // the whole column belongs to the shell
            for (int kk = k0; kk <= k1; kk++) md_visit(row + kk, p, tri, start, pairs, n_pairs, nf, B);
          } else {                                                              // only its two ends do (r >= 1 here)
            if (c[2] - r >= 0) md_visit(row + c[2] - r, p, tri, start, pairs, n_pairs, nf, B);
            if (c[2] + r <= G.n[2] - 1) md_visit(row + c[2] + r, p, tri, start, pairs, n_pairs, nf, B);
          }
        }
      }
      if (r == rmax) break;
      // the least distance from p to anything listed in no cell of the block [c - r, c + r]
      double bound = (double)INFINITY;
#pragma unroll
      for (int d = 0; d < 3; d++) {
        if (c[d] + r < G.n[d] - 1) {
          double e = ((double)G.lo[d] + ((double)(c[d] + r + 1) * shrink) * h) - p[d];
          e = e > 0.0 ? e : 0.0;
          bound = e < bound ? e : bound;
        }
        if (c[d] - r >= 1) {
          double e = p[d] - ((double)G.lo[d] + ((double)(c[d] - r) * grow) * h);
          e = e > 0.0 ? e : 0.0;
          bound = e < bound ? e : bound;
        }
      }
      if (bound * bound > B.d2) break;
    }
  }
  dist[i] = fin ? (float)sqrt(B.d2) : __builtin_nanf("");
  if (face) face[i] = B.face;
  if (bary) { bary[(size_t)i * 3] = (float)B.u; bary[(size_t)i * 3 + 1] = (float)B.v; bary[(size_t)i * 3 + 2] = (float)B.w; }
  if (closest) {
    if (B.face >= 0) {
      const float4 A = tri[3 * (size_t)B.face], Bc = tri[3 * (size_t)B.face + 1], C = tri[3 * (size_t)B.face + 2];
      closest[(size_t)i * 3] = (float)((B.u * (double)A.x + B.v * (double)Bc.x) + B.w * (double)C.x);
      closest[(size_t)i * 3 + 1] = (float)((B.u * (double)A.y + B.v * (double)Bc.y) + B.w * (double)C.y);
      closest[(size_t)i * 3 + 2] = (float)((B.u * (double)A.z + B.v * (double)Bc.z) + B.w * (double)C.z);
    } else {                                                                    // the point's own bits, NaN payloads included
      const uint32_t *src = reinterpret_cast<const uint32_t *>(points);
      uint32_t *dst = reinterpret_cast<uint32_t *>(closest);
#pragma unroll
      for (int d = 0; d < 3; d++) dst[(size_t)i * 3 + d] = src[(size_t)i * 3 + d];
    }
  }
  if (tests) tests[i] = B.tests;
}

__global__ __launch_bounds__(IA_MD_THREADS) void k_md_sample(const float *__restrict__ verts, const int32_t *__restrict__ faces, int nv, int nf,
                                                             const double *__restrict__ cum, int n, float *__restrict__ points,
                                                             int32_t *__restrict__ face, float *__restrict__ bary) {
  const long long i = (long long)blockIdx.x * IA_MD_THREADS + threadIdx.x;
  if (i >= n) return;
  const double A = cum[nf - 1];
  const double t = (((double)i + 0.5) / (double)n) * A;
  int lo = 0, hi = nf - 1;                               // the first f with cum[f] > t; nf - 1 when there is none
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (cum[mid] > t) hi = mid; else lo = mid + 1;
  }
  const int f = lo;
  const double a1 = 1.0 / IA_MESHDIST_PLASTIC, a2 = 1.0 / (IA_MESHDIST_PLASTIC * IA_MESHDIST_PLASTIC);
  double r1 = 0.5 + (double)i * a1, r2 = 0.5 + (double)i * a2;
  r1 = r1 - floor(r1); r2 = r2 - floor(r2);
  if (r1 + r2 > 1.0) { r1 = 1.0 - r1; r2 = 1.0 - r2; }
  float p[3][3];
  double nn[3];
  const bool ok = md_face(verts, faces, f, nv, p, nn);
  face[i] = ok ? f : -1;
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const double p0 = (double)p[0][d];
    points[(size_t)i * 3 + d] = ok ? (float)((p0 + r1 * ((double)p[1][d] - p0)) + r2 * ((double)p[2][d] - p0)) : __builtin_nanf("");
  }
  bary[(size_t)i * 3] = ok ? (float)((1.0 - r1) - r2) : 0.f;
  bary[(size_t)i * 3 + 1] = ok ? (float)r1 : 0.f;
  bary[(size_t)i * 3 + 2] = ok ? (float)r2 : 0.f;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------
extern "C" size_t ia_meshdist_grid_workspace_bytes(int nf, long long n_cells, long long n_pairs) {
  if (nf < 0 || nf > IA_MESHDIST_MAX_FACES || n_cells < 1 || n_cells > IA_MESHDIST_MAX_CELLS || n_pairs < 0 || n_pairs > IA_MESHDIST_MAX_PAIRS)
    return 0;
  return md_carve(nullptr, nf, n_cells, n_pairs).bytes;
}

extern "C" int ia_meshdist_grid_count(const float *verts, const int32_t *faces, int nv, int nf, float lo_x, float lo_y, float lo_z, float hi_x,
                                      float hi_y, float hi_z, float h, float inv_h, long long *n_pairs, void *stream) {
  const float lo[3] = {lo_x, lo_y, lo_z}, hi[3] = {hi_x, hi_y, hi_z};
  IaGrid G;
  long long cells;
  const int rc = md_check("ia_meshdist_grid_count", nf, lo, hi, h, inv_h, &G, &cells);
  if (rc) return rc;
  IA_CHECK_ARG(nv >= 0, "ia_meshdist_grid_count: nv = %d < 0", nv);
  IA_CHECK_ARG(n_pairs && (nf == 0 || (faces && (nv == 0 || verts))), "ia_meshdist_grid_count: null pointer");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_md_zero64, dim3(1), dim3(IA_MD_THREADS), 0, s, reinterpret_cast<unsigned long long *>(n_pairs));
  if (nf > 0)
    hipLaunchKernelGGL(k_md_count, dim3(ia_div_up(nf, IA_MD_THREADS)), dim3(IA_MD_THREADS), 0, s, verts, faces, nv, nf, G,
                       reinterpret_cast<unsigned long long *>(n_pairs));
  IA_LAUNCH_CHECK("k_md_count");
  return IA_OK;
}

extern "C" int ia_meshdist_grid_build(const float *verts, const int32_t *faces, int nv, int nf, float lo_x, float lo_y, float lo_z, float hi_x,
                                      float hi_y, float hi_z, float h, float inv_h, long long n_pairs, void *ws, size_t ws_bytes, void *stream) {
  const float lo[3] = {lo_x, lo_y, lo_z}, hi[3] = {hi_x, hi_y, hi_z};
  IaGrid G;
  long long cells;
  const int rc = md_check("ia_meshdist_grid_build", nf, lo, hi, h, inv_h, &G, &cells);
  if (rc) return rc;
  IA_CHECK_ARG(nv >= 0, "ia_meshdist_grid_build: nv = %d < 0", nv);
  IA_CHECK_ARG(n_pairs >= 0 && n_pairs <= IA_MESHDIST_MAX_PAIRS, "ia_meshdist_grid_build: n_pairs = %lld outside [0, %lld]: enlarge h", n_pairs,
               IA_MESHDIST_MAX_PAIRS);
  IA_CHECK_ARG(ws && (nf == 0 || (faces && (nv == 0 || verts))), "ia_meshdist_grid_build: null pointer");
  const MdWs W = md_carve(ws, nf, cells, n_pairs);
  if (ws_bytes < W.bytes) return ia_set_error(IA_ERR_WORKSPACE, "ia_meshdist_grid_build: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const dim3 b(IA_MD_THREADS);
  ia_fill_i32(W.cnt, cells, 0, s);
  if (nf > 0)
    hipLaunchKernelGGL(k_md_emit, dim3(ia_div_up(nf, IA_MD_THREADS)), b, 0, s, verts, faces, nv, nf, G, 0, W.tri, W.cnt, (const int32_t *)W.start, W.pairs, n_pairs);
  ia_scan(LoadInt{W.cnt}, cells, W.bsum, W.start, nullptr, s);
  ia_fill_i32(W.cnt, cells, 0, s);
  if (nf > 0)
    hipLaunchKernelGGL(k_md_emit, dim3(ia_div_up(nf, IA_MD_THREADS)), b, 0, s, verts, faces, nv, nf, G, 1, W.tri, W.cnt, (const int32_t *)W.start, W.pairs, n_pairs);
  IA_LAUNCH_CHECK("k_md_emit");
  return IA_OK;
}

extern "C" int ia_meshdist_closest(const float *points, int P, int nf, float lo_x, float lo_y, float lo_z, float hi_x, float hi_y, float hi_z,
                                   float h, float inv_h, long long n_pairs, const void *ws, size_t ws_bytes, float *dist, int32_t *face,
                                   float *bary, float *closest, int32_t *tests, void *stream) {
  const float lo[3] = {lo_x, lo_y, lo_z}, hi[3] = {hi_x, hi_y, hi_z};
  IaGrid G;
  long long cells;
  const int rc = md_check("ia_meshdist_closest", nf, lo, hi, h, inv_h, &G, &cells);
  if (rc) return rc;
  IA_CHECK_ARG(P >= 0, "ia_meshdist_closest: P = %d < 0", P);
  IA_CHECK_ARG(n_pairs >= 0 && n_pairs <= IA_MESHDIST_MAX_PAIRS, "ia_meshdist_closest: n_pairs = %lld outside [0, %lld]", n_pairs,
               IA_MESHDIST_MAX_PAIRS);
  if (P == 0) return IA_OK;
  IA_CHECK_ARG(points && dist && ws, "ia_meshdist_closest: null pointer");
  const MdWs W = md_carve(const_cast<void *>(ws), nf, cells, n_pairs);
  if (ws_bytes < W.bytes) return ia_set_error(IA_ERR_WORKSPACE, "ia_meshdist_closest: workspace too small");
  hipLaunchKernelGGL(k_md_closest, dim3(ia_div_up(P, IA_MD_THREADS)), dim3(IA_MD_THREADS), 0, (hipStream_t)stream, points, P, nf, G, n_pairs,
                     (const float4 *)W.tri, (const int32_t *)W.start, (const int32_t *)W.pairs, dist, face, bary, closest, tests);
  IA_LAUNCH_CHECK("k_md_closest");
  return IA_OK;
}

extern "C" int ia_meshdist_sample(const float *verts, const int32_t *faces, int nv, int nf, const double *cum, int n, float *points,
                                  int32_t *face, float *bary, void *stream) {
  IA_CHECK_ARG(nv >= 0 && nf >= 0 && n >= 0, "ia_meshdist_sample: negative size (nv = %d, nf = %d, n = %d)", nv, nf, n);
  if (n == 0) return IA_OK;
  IA_CHECK_ARG(nf >= 1 && nv >= 1, "ia_meshdist_sample: %d samples of a mesh without faces", n);
  IA_CHECK_ARG(verts && faces && cum && points && face && bary, "ia_meshdist_sample: null pointer");
  hipLaunchKernelGGL(k_md_sample, dim3(ia_div_up(n, IA_MD_THREADS)), dim3(IA_MD_THREADS), 0, (hipStream_t)stream, verts, faces, nv, nf, cum, n, points, face, bary);
  IA_LAUNCH_CHECK("k_md_sample");
  return IA_OK;
}
