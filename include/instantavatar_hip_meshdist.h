/*
 * instantavatar_hip_meshdist.h -- surface-distance entry points of libinstantavatar_hip.so (csrc/ia_meshdist.hip): a uniform grid of
 * triangles, the closest point of a triangle mesh for many query points, deterministic surface samples.  Conventions as in
 * instantavatar_hip.h (device pointers, `stream` as void*, no synchronisation, no allocation, scratch through `ws`, 0 = IA_OK); a
 * header of its own, bound by `_lib` as a table of its own.  Definitions: DESIGN.md section 4, "surface distance".
 *
 * Common to all of them.  A face is VALID when its three indices lie in [0, nv), are pairwise different and name vertices whose
 * three coordinates are finite (as in instantavatar_hip_meshops.h), and when in addition n = (p1 - p0) x (p2 - p0), formed in fp64, is
 * finite and not the zero vector; every other face is ignored.  All geometry is fp64 on the fp32 inputs converted exactly, without
 * fused multiply-adds; integer atomics only count or hand out slots: two calls on the same input give the same output bytes.
 */
#ifndef INSTANTAVATAR_HIP_MESHDIST_H
#define INSTANTAVATAR_HIP_MESHDIST_H

#include "instantavatar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the triangle grid: a uniform grid over the box [lo, hi] with cell edge h > 0, all by value; inv_h must be fp32(1 / h) (checked:
 * the search's bound rests on it).  Cells per axis n_a = max(1, ceil((hi_a - lo_a) / h)) in fp64, n_cells = n_x n_y n_z <=
 * IA_MESHDIST_MAX_CELLS; cell of a coordinate, per axis: clamp((int)floorf((p_a - lo_a) * inv_h), 0, n_a - 1) in fp32, as the cluster grid of
 * instantavatar_hip_meshops.h; key = (i n_y + j) n_z + k.  Every valid face is listed in every cell of the block [cell(min corner),
 * cell(max corner)] of its axis-aligned box -- a (face, cell) PAIR each.  The cell function is monotone, so a face that is not listed
 * in a block of cells lies, along one axis, wholly beyond the coordinates that fall into the block; the fp32 formula may differ from the
 * geometric cell by a relative 3 x 2^-24 of (p_a - lo_a) / h, which the search subtracts from its bound rather than widening the lists.
 * ia_meshdist_grid_count: n_pairs (device, 1 x int64) = the number of pairs.  The caller reads it and sizes the workspace.
 * ia_meshdist_grid_build: fills ws (ia_meshdist_grid_workspace_bytes(nf, n_cells, n_pairs)) with a record of three corners per face,
 *   the cells' offsets and the cells' face lists (in no particular order: no result depends on it).  n_pairs: what the count gave,
 *   <= IA_MESHDIST_MAX_PAIRS; a list is never truncated -- a call beyond a cap is an argument error, and a slot past n_pairs is not
 *   written.                                                                                                                  */
#define IA_MESHDIST_MAX_CELLS 16777216ll
#define IA_MESHDIST_MAX_PAIRS 2147483647ll
#define IA_MESHDIST_MAX_FACES 357913941
size_t ia_meshdist_grid_workspace_bytes(int nf, long long n_cells, long long n_pairs);
int ia_meshdist_grid_count(const float *verts, const int32_t *faces, int nv, int nf, float lo_x, float lo_y, float lo_z, float hi_x,
                           float hi_y, float hi_z, float h, float inv_h, long long *n_pairs, void *stream);
int ia_meshdist_grid_build(const float *verts, const int32_t *faces, int nv, int nf, float lo_x, float lo_y, float lo_z, float hi_x,
                           float hi_y, float hi_z, float h, float inv_h, long long n_pairs, void *ws, size_t ws_bytes, void *stream);

/* ---- closest point of the mesh for P query points [P,3]; the mesh is read from the grid's face records (same nf, box, h, inv_h, n_pairs
 * and ws as ia_meshdist_grid_build).
 *   - for a face, c = the closest point of the triangle by the Voronoi-region classification (Ericson, Real-Time Collision Detection
 *     5.1.5) in fp64: barycentrics (u, v, w) with exact zeros in the vertex and edge regions, u = 1 - v - w in the face region,
 *     c = (u p0 + v p1) + w p2, d2 = |p - c|^2 summed x, y, z;
 *   - the result of a point is the face with the lexicographically smallest (d2, face index) over ALL valid faces.  The grid only
 *     prunes: cells are visited in shells of Chebyshev radius r = 0, 1, ... around the point's cell, and the walk ends only when every
 *     face not yet seen is provably farther than the best so far (or every cell was seen), so no output but `tests` depends on the
 *     grid, on the order of a cell's list or on scheduling;
 *   - dist [P] = fp32(sqrt(d2)); face [P]; bary [P,3] = fp32(u, v, w); closest [P,3] = fp32(c); tests [P] = the number of
 *     point-triangle evaluations made for the point.  face, bary, closest and tests may be NULL;
 *   - a point with a non-finite coordinate: dist = NaN, face = -1, bary = 0, closest = the point, tests = 0;
 *   - a mesh without valid faces: dist = +inf, face = -1, bary = 0, closest = the point.                                      */
int ia_meshdist_closest(const float *points, int P, int nf, float lo_x, float lo_y, float lo_z, float hi_x, float hi_y, float hi_z,
                        float h, float inv_h, long long n_pairs, const void *ws, size_t ws_bytes, float *dist, int32_t *face,
                        float *bary, float *closest, int32_t *tests, void *stream);

/* ---- n deterministic surface samples, stratified over the area, no random generator.  cum [nf] (device, fp64): the inclusive prefix
 * sum of the face areas |n| / 2 in fp64, 0 for ignored faces; A = cum[nf - 1] (the caller refuses A = 0 or not finite).  Sample i:
 * t = ((i + 1/2) / n) A; its face = the first f with cum[f] > t (binary search; nf - 1 when there is none); r1 = frac(1/2 + i a1),
 * r2 = frac(1/2 + i a2) with a1 = 1 / g, a2 = 1 / (g g), g = IA_MESHDIST_PLASTIC (the R2 sequence), frac(x) = x - floor(x); when
 * r1 + r2 > 1 both become 1 - r; points [n,3] = fp32((p0 + r1 (p1 - p0)) + r2 (p2 - p0)), face [n], bary [n,3] = fp32(1 - r1 - r2,
 * r1, r2), all in fp64.  A face that cum selects although it is not valid gives face = -1, a NaN point and bary = 0.           */
#define IA_MESHDIST_PLASTIC 1.32471795724474602596
int ia_meshdist_sample(const float *verts, const int32_t *faces, int nv, int nf, const double *cum, int n, float *points,
                       int32_t *face, float *bary, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_MESHDIST_H */
