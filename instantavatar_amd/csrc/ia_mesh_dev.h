// ia_mesh_dev.h -- what the mesh units (ia_isosurface, ia_meshops, ia_meshdist, ia_meshray, ia_texture, ia_phototex, ia_scene) share: the pieces a
// face's validity is composed of, the fp64 face normal, the uniform grid of cells, the triangle grid's workspace and the layout of the texture atlas.  No kernel
// lives here; everything has internal linkage, so every unit that includes the header compiles its own copy of what it calls.
// The build has -ffp-contract=off: each function below is one fixed sequence of IEEE operations.
#pragma once
#include "ia_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// faces.  Every caller composes its own rule of validity from these pieces:
//   largest component      in range                                              (others are ignored)
//   clustering, adjacency  in range, distinct, the three `vok` bytes
//   surface distance       in range, distinct, finite corners, n finite and not zero
//   atlas, photo texture   in range (finite corners are tested per frame)
// T is float or double: the corners as they are stored, or widened (exactly) on the load
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ia_face_load(const int32_t *__restrict__ faces, int f, int v[3]) {
#pragma unroll
  for (int e = 0; e < 3; e++) v[e] = faces[(size_t)f * 3 + e];
}
__device__ __forceinline__ bool ia_face_in_range(const int v[3], int nv) {      // nv >= 0: a negative index is a large unsigned one
  return (uint32_t)v[0] < (uint32_t)nv && (uint32_t)v[1] < (uint32_t)nv && (uint32_t)v[2] < (uint32_t)nv;
}
__device__ __forceinline__ bool ia_face_distinct(const int v[3]) { return v[0] != v[1] && v[1] != v[2] && v[0] != v[2]; }

template <class T>
__device__ __forceinline__ void ia_face_corners(const float *__restrict__ verts, const int v[3], T p[3][3]) {
#pragma unroll
  for (int e = 0; e < 3; e++)
#pragma unroll
    for (int d = 0; d < 3; d++) p[e][d] = (T)verts[(size_t)v[e] * 3 + d];
}
template <class T>
__device__ __forceinline__ bool ia_finite3(T x, T y, T z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }
template <class T>
__device__ __forceinline__ bool ia_corners_finite(const T p[3][3]) {
  return ia_finite3(p[0][0], p[0][1], p[0][2]) && ia_finite3(p[1][0], p[1][1], p[1][2]) && ia_finite3(p[2][0], p[2][1], p[2][2]);
}

// n = (p1 - p0) x (p2 - p0) in fp64
template <class T>
__device__ __forceinline__ void ia_face_cross(const T p[3][3], double n[3]) {
  const double u0 = (double)p[1][0] - (double)p[0][0], u1 = (double)p[1][1] - (double)p[0][1], u2 = (double)p[1][2] - (double)p[0][2];
  const double w0 = (double)p[2][0] - (double)p[0][0], w1 = (double)p[2][1] - (double)p[0][1], w2 = (double)p[2][2] - (double)p[0][2];
  n[0] = u1 * w2 - u2 * w1; n[1] = u2 * w0 - u0 * w2; n[2] = u0 * w1 - u1 * w0;
}
__device__ __forceinline__ double ia_dot3d(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ double ia_len3d(const double n[3]) { return sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]); }

// ---------------------------------------------------------------------------------------------------------------------
// the uniform grid of cubic cells over a box (vertex clustering, surface distance)
// ---------------------------------------------------------------------------------------------------------------------
struct IaGrid { float lo[3]; float h, inv_h; int n[3]; };

// cell of a coordinate along one axis: clamp((int)floorf((p - lo) * inv_h), 0, n - 1), the clamp taken on the float so that no
// conversion leaves the range of int; NaN goes to 0.  Monotone in p.
__device__ __forceinline__ int ia_grid_cell(float p, float lo, float inv_h, int n) {
  const float t = floorf((p - lo) * inv_h);
  if (!(t > 0.f)) return 0;
  if (t >= (float)(n - 1)) return n - 1;
  return (int)t;
}

// the box and the cell edge, checked for entry point `who`; the grid and its number of cells.  max_text: max_cells as the messages
// print it; inv_exact: inv_h has to be fp32(1 / h), not only positive and finite
inline int ia_grid_check(const char *who, const float lo[3], const float hi[3], float h, float inv_h, bool inv_exact, long long max_cells,
                         const char *max_text, IaGrid *G, long long *cells) {
  IA_CHECK_ARG(h > 0.f && h < INFINITY, "%s: the cell edge h = %g must be positive and finite", who, (double)h);
  if (inv_exact)
    IA_CHECK_ARG(inv_h == (float)(1.0 / (double)h) && inv_h > 0.f && inv_h < INFINITY, "%s: inv_h = %g is not fp32(1 / h) = %g, positive and finite",
                 who, (double)inv_h, 1.0 / (double)h);
  IA_CHECK_ARG(inv_h > 0.f && inv_h < INFINITY, "%s: inv_h = %g must be positive and finite", who, (double)inv_h);
  double total = 1.0;
  for (int d = 0; d < 3; d++) {
    IA_CHECK_ARG(fabsf(lo[d]) < INFINITY && fabsf(hi[d]) < INFINITY, "%s: the box is not finite", who);
    double n = ceil(((double)hi[d] - (double)lo[d]) / (double)h);
    if (!(n >= 1.0)) n = 1.0;
    IA_CHECK_ARG(n <= (double)max_cells, "%s: a grid of more than %s cells (axis %d alone has %.0f): enlarge h", who, max_text, d, n);
    G->lo[d] = lo[d];
    G->n[d] = (int)n;
    total *= n;
  }
  IA_CHECK_ARG(total <= (double)max_cells, "%s: a grid of %d x %d x %d cells is more than %s: enlarge h", who, G->n[0], G->n[1], G->n[2],
               max_text);
  G->h = h;
  G->inv_h = inv_h;
  *cells = (long long)G->n[0] * G->n[1] * G->n[2];
  return IA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the triangle grid (ia_meshdist.hip builds it; ia_meshdist.hip and ia_meshray.hip read it)
// ---------------------------------------------------------------------------------------------------------------------
// the block of cells a face is listed in: per axis [cell(min corner), cell(max corner)]
__device__ __forceinline__ void md_range(const IaGrid &G, const float p[3][3], int c0[3], int c1[3]) {
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const float a = fminf(p[0][d], fminf(p[1][d], p[2][d])), b = fmaxf(p[0][d], fmaxf(p[1][d], p[2][d]));
    c0[d] = ia_grid_cell(a, G.lo[d], G.inv_h, G.n[d]);
    c1[d] = ia_grid_cell(b, G.lo[d], G.inv_h, G.n[d]);
  }
}

// the layout of its workspace: a record of three corners per face (NaN for a face that is not valid), the cells' offsets, counts and
// block sums (workgroups of IA_MD_THREADS = ia_scan.h's), the cells' face lists
#define IA_MD_THREADS 256
struct MdWs { float4 *tri; int32_t *start, *cnt, *bsum, *pairs; size_t bytes; };
inline MdWs md_carve(void *ws, int nf, long long cells, long long n_pairs) {
  WsCarver w(ws, 0);
  MdWs o;
  const size_t f = (size_t)(nf > 0 ? nf : 1), c = (size_t)(cells > 0 ? cells : 1);
  o.tri = w.take<float4>(3 * f);
  o.start = w.take<int32_t>(c + 1);
  o.cnt = w.take<int32_t>(c);
  o.bsum = w.take<int32_t>((size_t)ia_div_up((long long)c, IA_MD_THREADS) + 1);
  o.pairs = w.take<int32_t>((size_t)(n_pairs > 0 ? n_pairs : 1));
  o.bytes = w.off;
  return o;
}

// ---------------------------------------------------------------------------------------------------------------------
// the texture atlas: square blocks of B x B texels, nb per row, two faces per block.  Face 2 q + h owns half h of block q: half 0
// the texels with i + j <= B - 2, half 1 the others, seen from the opposite corner.  ia_texture.hip bakes through this mapping and
// ia_phototex.hip projects through it: one text, so the two agree bit for bit.
// ---------------------------------------------------------------------------------------------------------------------
// texel (i, j) of a block -> the half that owns it; (i, j) become the texel's coordinates in that half's own frame
__device__ __forceinline__ int ia_atlas_half(int B, int &i, int &j) {
  const int h = i + j <= B - 2 ? 0 : 1;
  if (h) {
    i = B - 1 - i;
    j = B - 1 - j;
  }
  return h;
}
__device__ __forceinline__ int ia_atlas_face(int br, int bc, int nb, int h) { return 2 * (br * nb + bc) + h; }   // < 2 nb^2 <= 2^25
// barycentric weights of the texel (i, j) of a half: corner 1 sits at i = B - 3, corner 2 at j = B - 3
__device__ __forceinline__ void ia_atlas_weights(int B, int i, int j, double u[3]) {
  const double L = (double)(B - 3);
  u[1] = (double)i / L;
  u[2] = (double)j / L;
  u[0] = 1.0 - u[1] - u[2];
}
// the point with weights u on the face with corners p, per axis u0 a + u1 b + u2 c from the left
__device__ __forceinline__ void ia_face_point(const double p[3][3], const double u[3], double x[3]) {
#pragma unroll
  for (int d = 0; d < 3; d++) x[d] = u[0] * p[0][d] + u[1] * p[1][d] + u[2] * p[2][d];
}

}  // namespace
