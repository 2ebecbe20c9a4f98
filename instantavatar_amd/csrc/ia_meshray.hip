// ia_meshray.hip -- rays against a triangle mesh (no counterpart in the reference): a walk of each ray through the triangle grid that
// ia_meshdist_grid_build makes.
//   one lane per ray: the first hit, the smallest (t, face) over all valid faces that are hit        (ia_meshray_closest)
//   one lane per ray: the number of valid faces that are hit, up to a limit (1: any-hit)             (ia_meshray_count)
// The definitions -- the hit of one face with its box clause, the outputs -- are stated in DESIGN.md section 4 ("ray queries") and in
// include/instantavatar_hip_meshray.h.  Nothing here synchronises, allocates or reads on the host; no LDS, no atomics.
//
// Why the result does not depend on the grid.  Whether a face is hit, and at which t, is one fixed fp64 expression of the ray and the
// face's corners (mr_hit): it knows nothing of the grid or of the walk.  The walk only has to EVALUATE every face that is hit.
//   (1) [t_min, t_max] is cut at an increasing sequence t_0 <= t_1 <= ... of parameters: the crossings of the grid's planes, in fp64,
//       ordered by a DDA.  Nothing below depends on where the cuts are, only on their order and on t_0 = the start, t_last = the end.
//   (2) For an interval [t_k, t_k+1] the walk forms c_a(t) = o_a + t d_a at both ends by the same two fp64 operations as the hit test.
//       A rounded product and a rounded sum are monotone in t, so c_a(t) of every t of the interval lies between the two values.
//   (3) It visits the BLOCK of cells from ia_grid_cell(rd32(smaller end)) to ia_grid_cell(ru32(larger end)) per axis -- the fp32,
//       clamped, monotone cell function the lists were built with (rd32 / ru32: the next fp32 below / above a double).
// A face hit at a t of the interval has, by the box clause, min_a <= ru32(c_a(t)) and rd32(c_a(t)) <= max_a; rd32, ru32 and the cell
// function are monotone, so cell(min_a) <= cell(ru32(larger end)) and cell(max_a) >= cell(rd32(smaller end)): the face's listed range
// [cell(min_a), cell(max_a)] meets the block's on every axis, and the face is listed in a cell of the block.  No epsilon appears.
// The cell function clamps, so boundary cells own everything outside the box and a ray outside the box needs no special case.  An
// unbounded last interval takes its far end as +-inf by the sign of d_a, or o_a when d_a = 0, and never forms inf * 0.
//
// Each cell is visited once.  Per axis both ends of the blocks' ranges move monotonically with k (c_a(t_k) is monotone in k), so a
// cell that lies in block j and in block k > j lies in every block between them; the walk skips the cells of block k that lie in
// block k - 1, and so evaluates a cell's list exactly when the cell first appears.  A skipped cell's faces were evaluated before, with
// the same expression over the whole range [t_min, t_max]: skipping loses nothing.
//   first hit: after interval k every face hit at some t <= t_k+1 has been evaluated (its t lies in an interval j <= k, it is listed in
//     block j).  The walk stops once best t <= t_k+1: every face not yet evaluated is hit, if at all, at t > t_k+1 >= best t, so it can
//     neither win nor tie.  The intervals are closed: a hit at exactly t_k+1 belongs to interval k already.
//   count: a face listed in several cells is counted in one canonical cell only: per axis ia_grid_cell(rd32(c_a)) of its hit point,
//     clamped into the face's own listed range (md_range recomputes it from the record's corners).  That cell lies in the block of the
//     interval that holds t (rd32(c_a) lies between the block's ends; the listed range meets the block, and clamping a member of one
//     range into another range that meets it gives a member of both), the face is listed there, and the cell is visited once: each
//     face that is hit is counted exactly once.  With limit = 1 the first hit met in any cell ends the walk.
//   faces_inside: with every corner inside [lo, hi], a hit has ru32(c_a) >= lo_a and rd32(c_a) <= hi_a.  The walk starts at a
//     candidate t_s > t_min only after CHECKING ru32(c_a(t_s)) < lo_a (d_a > 0; mirrored otherwise) with the hit test's own two
//     operations: by monotonicity no t <= t_s can be a hit.  The end is clipped the same way.  A candidate that fails its check is
//     dropped, so the rounding of the candidate itself does not matter.
#include "ia_common.h"
#include "ia_mesh_dev.h"
#include "../../include/instantavatar_hip_meshdist.h"
#include "../../include/instantavatar_hip_meshray.h"

#define IA_MR_THREADS 256

namespace {

// the next fp32 above / below f (f not NaN); an infinity on its own side stays
__device__ __forceinline__ float mr_up(float f) {
  if (f == INFINITY) return f;
  if (f == 0.f) return __uint_as_float(1u);
  const uint32_t b = __float_as_uint(f);
  return __uint_as_float((b >> 31) ? b - 1u : b + 1u);
}
__device__ __forceinline__ float mr_down(float f) {
  if (f == -INFINITY) return f;
  if (f == 0.f) return __uint_as_float(0x80000001u);
  const uint32_t b = __float_as_uint(f);
  return __uint_as_float((b >> 31) ? b + 1u : b - 1u);
}
// the largest fp32 not above / the smallest fp32 not below x (x not NaN)
__device__ __forceinline__ float mr_rd32(double x) {
  const float f = (float)x;
  return (double)f > x ? mr_down(f) : f;
}
__device__ __forceinline__ float mr_ru32(double x) {
  const float f = (float)x;
  return (double)f < x ? mr_up(f) : f;
}

struct MrRay { double o[3], d[3], t0, t1; };
struct MrBox { float hi[3]; };

// c_a(t) as the hit test forms it; for d_a = 0 it is o_a for every t, the infinite one included (no inf * 0)
__device__ __forceinline__ double mr_at(const MrRay &R, int a, double t) { return R.d[a] == 0.0 ? R.o[a] : R.o[a] + t * R.d[a]; }

// the hit of one face (the header's definition, operation by operation); t, u, v and the hit point c are only meaningful on a hit
__device__ __forceinline__ bool mr_hit(const MrRay &R, const float4 A, const float4 B, const float4 C, double &t, double &u, double &v,
                                       double c[3]) {
  const double p0[3] = {(double)A.x, (double)A.y, (double)A.z};
  const double e1[3] = {(double)B.x - p0[0], (double)B.y - p0[1], (double)B.z - p0[2]};
  const double e2[3] = {(double)C.x - p0[0], (double)C.y - p0[1], (double)C.z - p0[2]};
  const double pv[3] = {R.d[1] * e2[2] - R.d[2] * e2[1], R.d[2] * e2[0] - R.d[0] * e2[2], R.d[0] * e2[1] - R.d[1] * e2[0]};
  const double det = ia_dot3d(e1, pv);
  const double inv = 1.0 / det;
  const double tv[3] = {R.o[0] - p0[0], R.o[1] - p0[1], R.o[2] - p0[2]};
  u = ia_dot3d(tv, pv) * inv;
  const double qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
  v = ia_dot3d(R.d, qv) * inv;
  const double w = (1.0 - u) - v;
  t = ia_dot3d(e2, qv) * inv;
  if (!(det != 0.0)) return false;
  if (!(u >= 0.0 && v >= 0.0 && w >= 0.0)) return false;
  if (!(__builtin_isfinite(t) && R.t0 <= t && t <= R.t1)) return false;
  const float pa[3] = {A.x, A.y, A.z}, pb[3] = {B.x, B.y, B.z}, pc[3] = {C.x, C.y, C.z};
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    c[a] = R.o[a] + t * R.d[a];
    const float mn = fminf(pa[a], fminf(pb[a], pc[a])), mx = fmaxf(pa[a], fmaxf(pb[a], pc[a]));
    in = in && mr_rd32(c[a]) <= mx && mr_ru32(c[a]) >= mn;
  }
  return in;
}

// t of the crossing of plane i of axis a (i in 1 .. n_a - 1), +inf when the planes of the axis are used up
__device__ __forceinline__ double mr_plane_t(const MrRay &R, const IaGrid &G, int a, int i) {
  if (i < 1 || i > G.n[a] - 1) return (double)INFINITY;
  return (((double)G.lo[a] + (double)i * (double)G.h) - R.o[a]) / R.d[a];
}

template <int COUNT>
__global__ __launch_bounds__(IA_MR_THREADS) void k_mr_walk(const float *__restrict__ origins, const float *__restrict__ dirs,
                                                           const float *__restrict__ t_min, const float *__restrict__ t_max, int P, int nf,
                                                           IaGrid G, MrBox X, long long n_pairs, const float4 *__restrict__ tri,
                                                           const int32_t *__restrict__ start, const int32_t *__restrict__ pairs,
                                                           int faces_inside, int limit, float *__restrict__ t_out,
                                                           int32_t *__restrict__ face_out, float *__restrict__ bary,
                                                           int32_t *__restrict__ count_out, int32_t *__restrict__ tests) {
  const long long r = (long long)blockIdx.x * IA_MR_THREADS + threadIdx.x;
  if (r >= P) return;
  const float of[3] = {origins[(size_t)r * 3], origins[(size_t)r * 3 + 1], origins[(size_t)r * 3 + 2]};
  const float df[3] = {dirs[(size_t)r * 3], dirs[(size_t)r * 3 + 1], dirs[(size_t)r * 3 + 2]};
  const float t0f = t_min ? t_min[r] : 0.f, t1f = t_max ? t_max[r] : INFINITY;
  const bool valid = ia_finite3(of[0], of[1], of[2]) && ia_finite3(df[0], df[1], df[2]) && t0f >= 0.f && t0f <= t1f;
  double best_t = (double)INFINITY, best_u = 0.0, best_v = 0.0;
  int best_f = -1, n_tests = 0, cnt = 0;
  bool live = valid && (df[0] != 0.f || df[1] != 0.f || df[2] != 0.f) && t0f < INFINITY;      // a hit needs a finite t >= t_min, and det != 0
  if (live) {
    MrRay R;
#pragma unroll
    for (int a = 0; a < 3; a++) { R.o[a] = (double)of[a]; R.d[a] = (double)df[a]; }
    R.t0 = (double)t0f; R.t1 = (double)t1f;
    double ts = R.t0, te = R.t1;
    if (faces_inside) {
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const float lo = G.lo[a], hi = X.hi[a];
        if (R.d[a] == 0.0) {
          live = live && of[a] >= lo && of[a] <= hi;                                          // c_a = o_a for every t
          continue;
        }
        const bool pos = R.d[a] > 0.0;
        double cand = ((double)(pos ? mr_down(mr_down(lo)) : mr_up(mr_up(hi))) - R.o[a]) / R.d[a];
        if (cand > ts && cand < (double)INFINITY) {
          const double c = R.o[a] + cand * R.d[a];
          if (pos ? mr_ru32(c) < lo : mr_rd32(c) > hi) ts = cand;                             // no t <= cand is a hit
        }
        cand = ((double)(pos ? mr_up(mr_up(hi)) : mr_down(mr_down(lo))) - R.o[a]) / R.d[a];
        if (cand < te) {
          const double c = R.o[a] + cand * R.d[a];
          if (pos ? mr_rd32(c) > hi : mr_ru32(c) < lo) te = cand;                             // no t >= cand is a hit
        }
      }
      live = live && ts <= te;
    }
    if (live) {
      // the DDA over the planes of the three axes: ip = the next plane of the axis, tn = its parameter
      int ip[3];
      double tn[3], cprev[3];
#pragma unroll
      for (int a = 0; a < 3; a++) {
        cprev[a] = mr_at(R, a, ts);
        ip[a] = 0;
        tn[a] = (double)INFINITY;
        if (R.d[a] != 0.0) {
          const double g = (cprev[a] - (double)G.lo[a]) / (double)G.h;
          const bool pos = R.d[a] > 0.0;                                                      // planes 1 .. n - 1 cut; n / 0: none left
          const double fi = pos ? floor(g) + 1.0 : ceil(g) - 1.0;
          ip[a] = (int)fmin(fmax(fi, pos ? 1.0 : 0.0), (double)(pos ? G.n[a] : G.n[a] - 1));
          tn[a] = mr_plane_t(R, G, a, ip[a]);
        }
      }
      double ta = ts;
      int q0[3] = {0, 0, 0}, q1[3] = {-1, -1, -1};                                            // the previous block (empty at first)
      for (;;) {
        int ax = 0;
        double tb = tn[0];
        if (tn[1] < tb) { ax = 1; tb = tn[1]; }
        if (tn[2] < tb) { ax = 2; tb = tn[2]; }
        const bool last = !(tb < te);
        if (last) tb = te;
        else {
          ip[ax] += R.d[ax] > 0.0 ? 1 : -1;
          tn[ax] = mr_plane_t(R, G, ax, ip[ax]);
          if (tb < ta) tb = ta;                                                               // the sequence of cuts never decreases
        }
        int b0[3], b1[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
          const double cb = mr_at(R, a, tb);
          const double mn = cb < cprev[a] ? cb : cprev[a], mx = cb < cprev[a] ? cprev[a] : cb;
          b0[a] = ia_grid_cell(mr_rd32(mn), G.lo[a], G.inv_h, G.n[a]);
          b1[a] = ia_grid_cell(mr_ru32(mx), G.lo[a], G.inv_h, G.n[a]);
          cprev[a] = cb;
        }
        for (int i = b0[0]; i <= b1[0]; i++) {
          const bool old_i = i >= q0[0] && i <= q1[0];
          for (int j = b0[1]; j <= b1[1]; j++) {
            const bool old_j = old_i && j >= q0[1] && j <= q1[1];
            for (int k = b0[2]; k <= b1[2]; k++) {
              if (old_j && k >= q0[2] && k <= q1[2]) continue;                                // a cell of the previous block: done
              const long long key = ((long long)i * G.n[1] + j) * G.n[2] + k;
              const int s0 = start[key];
              long long s1 = start[key + 1];
              if (s1 > n_pairs) s1 = n_pairs;
              for (long long s = s0; s < s1; s++) {
                const int f = pairs[s];
                if ((uint32_t)f >= (uint32_t)nf) continue;                                    // (never for a list that grid_build made)
                const float4 A = tri[3 * (size_t)f], B = tri[3 * (size_t)f + 1], C = tri[3 * (size_t)f + 2];
                double t, u, v, c[3];
                n_tests++;
                if (!mr_hit(R, A, B, C, t, u, v, c)) continue;
                if (!COUNT) {
                  if (t < best_t || (t == best_t && f < best_f)) { best_t = t; best_u = u; best_v = v; best_f = f; }
                } else {
                  bool own = true;
                  if (limit != 1) {                                                           // the face's canonical cell
                    const float p[3][3] = {{A.x, A.y, A.z}, {B.x, B.y, B.z}, {C.x, C.y, C.z}};
                    int c0[3], c1[3];
                    md_range(G, p, c0, c1);
                    const int here[3] = {i, j, k};
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                      int cc = ia_grid_cell(mr_rd32(c[a]), G.lo[a], G.inv_h, G.n[a]);
                      cc = cc < c0[a] ? c0[a] : (cc > c1[a] ? c1[a] : cc);
                      own = own && cc == here[a];
                    }
                  }
                  if (own && ++cnt >= limit) goto done;
                }
              }
            }
          }
        }
        if (last) break;
        if (!COUNT && best_t <= tb) break;
#pragma unroll
        for (int a = 0; a < 3; a++) { q0[a] = b0[a]; q1[a] = b1[a]; }
        ta = tb;
      }
    }
  }
done:
  if (COUNT) {
    count_out[r] = valid ? cnt : -1;
  } else {
    t_out[r] = valid ? (float)best_t : __builtin_nanf("");
    if (face_out) face_out[r] = best_f;
    if (bary) {
      bary[(size_t)r * 3] = best_f >= 0 ? (float)((1.0 - best_u) - best_v) : 0.f;
      bary[(size_t)r * 3 + 1] = (float)best_u;
      bary[(size_t)r * 3 + 2] = (float)best_v;
    }
  }
  if (tests) tests[r] = n_tests;
}

// the arguments both entries share, checked; the grid, the box's far corner and the carved workspace
int mr_check(const char *who, int P, int nf, const float lo[3], const float hi[3], float h, float inv_h, long long n_pairs, const void *ws,
             size_t ws_bytes, int faces_inside, IaGrid *G, MrBox *X, MdWs *W) {
  IA_CHECK_ARG(P >= 0, "%s: P = %d < 0", who, P);
  IA_CHECK_ARG(nf >= 0 && nf <= IA_MESHDIST_MAX_FACES, "%s: nf = %d outside [0, %d]", who, nf, IA_MESHDIST_MAX_FACES);
  long long cells;
  const int rc = ia_grid_check(who, lo, hi, h, inv_h, true, IA_MESHDIST_MAX_CELLS, "16777216", G, &cells);
  if (rc) return rc;
  IA_CHECK_ARG(n_pairs >= 0 && n_pairs <= IA_MESHDIST_MAX_PAIRS, "%s: n_pairs = %lld outside [0, %lld]", who, n_pairs, IA_MESHDIST_MAX_PAIRS);
  IA_CHECK_ARG(faces_inside == 0 || faces_inside == 1, "%s: faces_inside = %d is neither 0 nor 1", who, faces_inside);
  for (int a = 0; a < 3; a++) X->hi[a] = hi[a];
  *W = md_carve(const_cast<void *>(ws), nf, cells, n_pairs);
  if (P > 0) {
    IA_CHECK_ARG(ws, "%s: null pointer", who);
    if (ws_bytes < W->bytes) return ia_set_error(IA_ERR_WORKSPACE, "%s: workspace too small", who);
  }
  return IA_OK;
}

}  // namespace

extern "C" int ia_meshray_closest(const float *origins, const float *dirs, const float *t_min, const float *t_max, int P, int nf, float lo_x,
                                  float lo_y, float lo_z, float hi_x, float hi_y, float hi_z, float h, float inv_h, long long n_pairs,
                                  const void *ws, size_t ws_bytes, int faces_inside, float *t, int32_t *face, float *bary, int32_t *tests,
                                  void *stream) {
  const float lo[3] = {lo_x, lo_y, lo_z}, hi[3] = {hi_x, hi_y, hi_z};
  IaGrid G;
  MrBox X;
  MdWs W;
  const int rc = mr_check("ia_meshray_closest", P, nf, lo, hi, h, inv_h, n_pairs, ws, ws_bytes, faces_inside, &G, &X, &W);
  if (rc) return rc;
  if (P == 0) return IA_OK;
  IA_CHECK_ARG(origins && dirs && t, "ia_meshray_closest: null pointer");
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mr_walk<0>), dim3(ia_div_up(P, IA_MR_THREADS)), dim3(IA_MR_THREADS), 0, (hipStream_t)stream, origins, dirs,
                     t_min, t_max, P, nf, G, X, n_pairs, (const float4 *)W.tri, (const int32_t *)W.start, (const int32_t *)W.pairs, faces_inside,
                     INT_MAX, t, face, bary, (int32_t *)nullptr, tests);
  IA_LAUNCH_CHECK("k_mr_walk");
  return IA_OK;
}

extern "C" int ia_meshray_count(const float *origins, const float *dirs, const float *t_min, const float *t_max, int P, int nf, float lo_x,
                                float lo_y, float lo_z, float hi_x, float hi_y, float hi_z, float h, float inv_h, long long n_pairs,
                                const void *ws, size_t ws_bytes, int faces_inside, int limit, int32_t *count, int32_t *tests, void *stream) {
  const float lo[3] = {lo_x, lo_y, lo_z}, hi[3] = {hi_x, hi_y, hi_z};
  IaGrid G;
  MrBox X;
  MdWs W;
  const int rc = mr_check("ia_meshray_count", P, nf, lo, hi, h, inv_h, n_pairs, ws, ws_bytes, faces_inside, &G, &X, &W);
  if (rc) return rc;
  IA_CHECK_ARG(limit >= 1, "ia_meshray_count: limit = %d < 1", limit);
  if (P == 0) return IA_OK;
  IA_CHECK_ARG(origins && dirs && count, "ia_meshray_count: null pointer");
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mr_walk<1>), dim3(ia_div_up(P, IA_MR_THREADS)), dim3(IA_MR_THREADS), 0, (hipStream_t)stream, origins, dirs,
                     t_min, t_max, P, nf, G, X, n_pairs, (const float4 *)W.tri, (const int32_t *)W.start, (const int32_t *)W.pairs, faces_inside,
                     limit, (float *)nullptr, (int32_t *)nullptr, (float *)nullptr, count, tests);
  IA_LAUNCH_CHECK("k_mr_walk");
  return IA_OK;
}
