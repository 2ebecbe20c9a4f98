/*
 * instantavatar_hip_silhouette.h -- the differentiable soft silhouette of a triangle mesh and the body-model adjoint that carries
 * its vertex cotangent to pose and translation (csrc/ia_silhouette.hip; the adjoint lives next to the kernels it shares, in
 * csrc/ia_keypoints.hip).  Conventions as in instantavatar_hip.h (device pointers, `stream` as void*, no allocation, scratch
 * through `ws`, 0 = IA_OK, no host synchronisation); a header of its own, bound by `_lib` as a seventh table.
 *
 * Definition ("silhouette refinement"; the `--silhouette` stage of scripts/custom/refine-smpl.py, whose
 * renderer is pytorch3d's soft rasteriser):
 *   camera     the OpenCV pinhole of raster.Camera: p = R X + t (w2c rows 0..2), u = fx p.x / p.z + cx, v = fy p.y / p.z + cy; pixel
 *              (x, y) is sampled AT (x, y), as make_rays and ia_raster_* do (pytorch3d's pixel centres sit at +0.5: a stated
 *              deviation)
 *   vertices   screen [nv,2] fp32 pixels, inv_z [nv] = 1 / p.z.  A vertex with p.z < near, a non-finite coordinate or |u|, |v| >
 *              IA_SIL_XY_MAX is invalid: screen = 0, inv_z = 0
 *   faces      skipped, nothing clipped, with an invalid vertex, an index outside [0, nv) or a doubled screen area
 *              A = (b - a) x (c - a) == 0 (fp32, products rounded separately): the rules of ia_raster_visibility
 *   distance   pixel P, face (a, b, c), edges k = 0, 1, 2 = a->b, b->c, c->a:  t = clamp((P - v_k) . e / |e|^2, 0, 1),
 *              q = P - (v_k + t e), dist2 = min_k |q|^2, the lower k winning an exact tie;  inside iff sign(A) (e x (P - v_k)) > 0 for
 *              all three;  d = dist2 (2 / min(H, W))^2  (pytorch3d's NDC: the short side spans [-1, 1])
 *   coverage   a face contributes to a pixel iff inside or d < blur_radius;  x_f = +d / sigma inside, -d / sigma outside;
 *              p_f = sigmoid(x_f);  alpha = 1 - prod_f (1 - p_f) over the contributing faces IN FACE ORDER, every face within the
 *              radius (no faces_per_pixel cap: the second stated deviation)
 *   loss       L = sum_pixels (alpha - m)^2 / (H W), m the mask in [0, 1];  d_alpha = 2 (alpha - m) / (H W)
 *   gradient   d alpha / d x_f = (1 - alpha) p_f;  d dist2 / d v_k = -2 (1 - t) q, d dist2 / d v_k+1 = -2 t q on the winning edge, t
 *              clamped or not;  the cut at blur_radius carries none
 * fp32, fixed-order sums and products, no floating-point atomics: two calls on the same inputs give the same bits.  Every output
 * element is written (zeros included); no buffer has to be zeroed by the caller and nothing has to survive in ws between calls.
 *
 * ia_sil_project_fwd: verts [nv,3], w2c [4,4] (device) -> screen [nv,2], inv_z [nv].
 * ia_sil_project_bwd: the same inputs and d_screen [nv,2] -> d_verts [nv,3]; an invalid vertex gets zeros.
 * ia_sil_workspace_bytes: scratch of the two render entries; 0 outside nv, nf >= 0, 3 nf < 2^31, 1 <= H, W <= IA_SIL_MAX_DIM.
 * ia_sil_render_fwd: screen, inv_z, faces [nf,3] (device int32), mask [H*W] or NULL -> alpha [H*W], loss [1], d_alpha [H*W]; each
 *   output may be NULL, loss and d_alpha need the mask.  sigma > 0, blur_radius >= 0, both finite.
 * ia_sil_render_bwd: the same inputs, alpha as the forward wrote it, d_alpha, and the vertex-to-face list of the topology --
 *   vf_start [nv+1] ascending offsets into vf_corner [vf_start[nv] <= 3 nf], whose entries 3 f + c name corner c of face f; the
 *   gather adds them in list order (entries or offsets outside their range are ignored, never dereferenced) -> d_screen [nv,2].
 * ia_sil_body_workspace_bytes / ia_sil_body_bwd: the adjoint of vert[f,v] = T_v (vs + po) + transl[f] exactly as ia_kp_loss_fwd
 *   defines it (instantavatar_hip_keypoints.h): betas [10], pose [F,72], transl [F,3], d_verts [F,V,3] -> d_betas [10],
 *   d_pose [F,72], d_transl [F,3]; each may be NULL.  0 bytes for n_frames < 1, n_verts < 1 or n_frames * n_verts * 3 >= 2^31. */
#ifndef INSTANTAVATAR_HIP_SILHOUETTE_H
#define INSTANTAVATAR_HIP_SILHOUETTE_H

#include "instantavatar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IA_SIL_MAX_DIM 16384
#define IA_SIL_XY_MAX 16384.0f
int ia_sil_project_fwd(const float *verts, int nv, const float *w2c, float fx, float fy, float cx, float cy, float near,
                       float *screen, float *inv_z, void *stream);
int ia_sil_project_bwd(const float *verts, int nv, const float *w2c, float fx, float fy, float cx, float cy, float near,
                       const float *d_screen, float *d_verts, void *stream);
size_t ia_sil_workspace_bytes(int nv, int nf, int H, int W);
int ia_sil_render_fwd(const float *screen, const float *inv_z, int nv, const int32_t *faces, int nf, int H, int W, float sigma,
                      float blur_radius, const float *mask, float *alpha, float *loss, float *d_alpha, void *ws, size_t ws_bytes,
                      void *stream);
int ia_sil_render_bwd(const float *screen, const float *inv_z, int nv, const int32_t *faces, int nf, int H, int W, float sigma,
                      float blur_radius, const float *alpha, const float *d_alpha, const int32_t *vf_start,
                      const int32_t *vf_corner, float *d_screen, void *ws, size_t ws_bytes, void *stream);
size_t ia_sil_body_workspace_bytes(int n_frames, int n_verts);
int ia_sil_body_bwd(const ia_smpl_body *body, const float *betas, const float *pose, const float *transl, int n_frames,
                    const float *d_verts, float *d_betas, float *d_pose, float *d_transl, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_SILHOUETTE_H */
