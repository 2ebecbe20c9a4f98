/*
 * instantavatar_hip_meshray.h -- ray-query entry points of libinstantavatar_hip.so (csrc/ia_meshray.hip): the first hit of many rays
 * with a triangle mesh, and the number of faces a ray hits (any-hit, parity).  Conventions as in instantavatar_hip.h (device pointers,
 * `stream` as void*, no synchronisation, no allocation, 0 = IA_OK); a header of its own, bound by `_lib` as a table of its own.
 * Definitions: DESIGN.md section 4, "ray queries".
 *
 * Common to both.  Validity of a face, "fp64" arithmetic and the grid are those of instantavatar_hip_meshdist.h: the fp32 inputs are
 * converted exactly, every operation is a separate IEEE double operation in the order written (no fused multiply-adds).  The mesh is
 * read from the face records of the triangle grid: nf, the box, h, inv_h, n_pairs, ws and ws_bytes are what ia_meshdist_grid_build
 * was given (inv_h must be fp32(1 / h), checked).
 *
 * A RAY is an origin o (origins [P,3]), a direction d (dirs [P,3]; not normalised: t counts in units of d) and a closed range
 * [t_min, t_max] with 0 <= t_min <= t_max <= +inf (t_min, t_max: [P] fp32 each, or NULL for 0 / +inf).  A ray is INVALID when a
 * coordinate of o or d is not finite, or when its range is NaN or violates that order.
 *
 * HIT OF ONE FACE with corners p0, p1, p2, in fp64, dot(a, b) = (a0 b0 + a1 b1) + a2 b2,
 * a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0):
 *     e1 = p1 - p0, e2 = p2 - p0, pv = d x e2, det = dot(e1, pv), inv = 1 / det, tv = o - p0,
 *     u = dot(tv, pv) * inv, qv = tv x e1, v = dot(d, qv) * inv, w = (1 - u) - v, t = dot(e2, qv) * inv, c_a = o_a + t * d_a.
 * The face is hit iff ALL of these hold (positive comparisons: a NaN anywhere is a miss):
 *     det != 0;  u >= 0, v >= 0, w >= 0;  t finite and t_min <= t <= t_max;
 *     the BOX CLAUSE: on every axis a, rd32(c_a) <= max_a and ru32(c_a) >= min_a, where min_a / max_a are the smallest / largest
 *     corner coordinate and rd32(x) / ru32(x) the largest fp32 not above / the smallest fp32 not below x.
 * Two-sided, no culling.  The box clause admits one fp32 ulp around the computed hit point -- orders of magnitude more than the fp64
 * rounding of c, so it rejects no geometric hit -- and is what makes the walk through the grid provably complete (ia_meshray.hip):
 * no output but `tests` depends on the grid, on the order of a cell's list, on the order of the rays or on scheduling.
 */
#ifndef INSTANTAVATAR_HIP_MESHRAY_H
#define INSTANTAVATAR_HIP_MESHRAY_H

#include "instantavatar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* faces_inside (both entries): 0, or 1 when the caller asserts that every corner of every valid face lies in the box [lo, hi] (true
 * when the box was derived from the valid faces' bounds).  The walk may then skip the parameters whose c lies outside the box widened by
 * one fp32 ulp.  A wrong assertion is the caller's error: hits outside the box may then be missed.
 *
 * ---- first hit: the face with the lexicographically smallest (t, face index) over ALL valid faces that are hit.
 *   - t [P] = fp32(t); face [P]; bary [P,3] = fp32(w, u, v), the weights of p0, p1, p2; tests [P] = the number of ray-triangle
 *     evaluations made for the ray.  face, bary and tests may be NULL;
 *   - no face is hit (d = 0 included): t = +inf, face = -1, bary = 0;
 *   - an invalid ray: t = NaN, face = -1, bary = 0, tests = 0.                                                                  */
int ia_meshray_closest(const float *origins, const float *dirs, const float *t_min, const float *t_max, int P, int nf, float lo_x,
                       float lo_y, float lo_z, float hi_x, float hi_y, float hi_z, float h, float inv_h, long long n_pairs,
                       const void *ws, size_t ws_bytes, int faces_inside, float *t, int32_t *face, float *bary, int32_t *tests,
                       void *stream);

/* ---- hit count: count [P] = min(limit, the number of valid faces that are hit), each face once; limit >= 1.  limit = 1 is the any-hit
 * query ("is the segment blocked?"): the walk ends at the first hit it meets.  An invalid ray: count = -1, tests = 0.  tests may be
 * NULL.                                                                                                                         */
int ia_meshray_count(const float *origins, const float *dirs, const float *t_min, const float *t_max, int P, int nf, float lo_x,
                     float lo_y, float lo_z, float hi_x, float hi_y, float hi_z, float h, float inv_h, long long n_pairs,
                     const void *ws, size_t ws_bytes, int faces_inside, int limit, int32_t *count, int32_t *tests, void *stream);

/* ---- the inside test (formed by the caller from the count): a point is the origin of three rays over [0, +inf] with the fixed fp32
 * directions below; it is INSIDE iff at least two of the three counts are odd.  This assumes a closed surface; the orientation of the
 * faces does not matter.  The directions are pairwise far from parallel (as lines, 75 degrees or more apart) and none lies within 10 degrees of a
 * coordinate axis, a coordinate plane or a cube diagonal: meshes from a lattice are full of axis-aligned edges, and a skewed ray does
 * not run along them.                                                                                                            */
#define IA_MESHRAY_INSIDE_DIR_0 0.90f, 0.35f, 0.26f
#define IA_MESHRAY_INSIDE_DIR_1 -0.30f, 0.85f, 0.43f
#define IA_MESHRAY_INSIDE_DIR_2 0.40f, 0.28f, -0.87f

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_MESHRAY_H */
