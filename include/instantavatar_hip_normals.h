/*
 * instantavatar_hip_normals.h -- the surface-normal entry points of libinstantavatar_hip.so (csrc/ia_normals.hip).
 * Conventions as in instantavatar_hip.h (device pointers, `stream` as void*, no synchronisation, no allocation, scratch
 * through `ws`, 0 = IA_OK); a header of its own, bound by `_lib` as a table of its own next to the main one.
 */
#ifndef INSTANTAVATAR_HIP_NORMALS_H
#define INSTANTAVATAR_HIP_NORMALS_H

#include "instantavatar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- surface normals of the posed density field (no counterpart in the reference: its geometry figures are normal maps) ----
 * A second pass over at most one point per pixel of a rendered frame.  Definition, for a pixel with
 * alpha >= 0.5 and a finite depth / alpha:
 *   1. surface point p = o + (depth / alpha) d, in the frame the marcher works in (after ia_transform_rays_w2s);
 *   2. p is deformed to canonical candidates as deform_test does (search, duplicate filter, field); the root x_c is the
 *      candidate with the largest sigma (first maximum; a non-finite sigma counts as 0); no valid candidate: no normal;
 *   3. g = d sigma / d x_c of the sigma network at x_c: fp16 table and weights, ReLU mask from the forward's half-rounded
 *      hidden layer, analytic derivative of the trilinear interpolation (ia_hashgrid_bwd's `dx`), 0 along an axis on which
 *      the field's clamp to its box is active; no finite differences;
 *   4. M = the 3x3 linear part of voxel_J interpolated at x_c; n = -M^{-T} g / |M^{-T} g|, rotated into the camera frame with
 *      the transpose of w2s' rotation.  The spatial derivative of the skinning weights (of M itself) is ignored.  g = 0, a
 *      singular M or a non-finite value give the zero vector, never NaN;
 *   5. the map is [R,3] fp32: zero where there is no normal, unit length elsewhere.
 *
 * ia_surface_points: compact list of the surface points IN RAY ORDER (ballot / prefix sums: deterministic): pts [<= R,3],
 *   ray_idx [<= R] the ray of every point, *n_pts (device) their number.  ws: ia_surface_points_workspace_bytes(R).
 * ia_field_sigma_grad: sigma [V] (bit for bit ia_field_fwd's) and grad [V,3] = d sigma / d x in ONE kernel; rows >= the live
 *   count (n_dev) are left untouched.  No table gradient, no activation record, no atomics.
 * ia_candidate_select: per point the candidate with the largest sigma (lists of ia_snarf_search_compact): root [P,3],
 *   grad [P,3] (zeros for a point without candidates), arg [P] (optional: its index in the candidate list, -1).
 * ia_normals_from_gradient: step 4 for n points (live: n_dev), scattered to normals [R,3] at ray_idx; the map is zero-filled
 *   by the call first (a kernel, not a memset).  w2s: DEVICE [4,4].
 * ia_pack_normals8: the two 8-bit images of a map in one launch: normal_rgba [R,4] = ((n + 1) / 2, covered), shaded_rgba
 *   [R,4] = (s, s, s, covered), s = max(0, n . l); l = light (DEVICE float[3], normalised by the call) or, when NULL, the
 *   direction towards the camera along the pixel's own ray (-rays_d [R,3], camera frame).  covered = 255 where the pixel has a
 *   normal; pixels without one are 0 in all channels.  Quantisation as ia_pack_rgba8.  Both images 4-byte aligned.     */
size_t ia_surface_points_workspace_bytes(int R);
int ia_surface_points(const float *rays_o, const float *rays_d, const float *depth, const float *alpha, int R,
                      float *pts, int32_t *ray_idx, int32_t *n_pts, void *ws, size_t ws_bytes, void *stream);
int ia_field_sigma_grad(const float *x, int V, const int32_t *n_dev, const ia_field *field, float *sigma, float *grad,
                        void *stream);
int ia_candidate_select(const float *cand_sigma, const float *cand_xc, const float *cand_grad, int cand_cap,
                        const int32_t *pt_off, const uint8_t *pt_cnt, int P, const int32_t *n_pts_dev, float *root,
                        float *grad, int32_t *arg, void *stream);
int ia_normals_from_gradient(const float *root, const float *grad, const int32_t *ray_idx, int n, const int32_t *n_dev,
                             const float *voxel_J, const ia_snarf_grid *grid, const float *w2s, int R, float *normals,
                             void *stream);
int ia_pack_normals8(const float *normals, const float *rays_d, const float *light, int R, uint8_t *normal_rgba,
                     uint8_t *shaded_rgba, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_NORMALS_H */
