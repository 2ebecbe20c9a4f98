/*
 * instantavatar_hip_keypoints.h -- the keypoint-refinement entry points of libinstantavatar_hip.so (csrc/ia_keypoints.hip).
 * Conventions as in instantavatar_hip.h (device pointers, `stream` as void*, no allocation, scratch through `ws`, 0 = IA_OK);
 * a header of its own, bound by `_lib` as a table of its own next to the other five.  ONE exception to "no synchronisation":
 * both loss entries wait for their first kernel, which validates the device copy of kp_vertex, before they launch anything
 * else (one 4-byte read-back per call), so an index outside the body is an argument error and never an out-of-bounds read.
 * They can therefore not be captured into a graph.
 */
#ifndef INSTANTAVATAR_HIP_KEYPOINTS_H
#define INSTANTAVATAR_HIP_KEYPOINTS_H

#include "instantavatar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the loss of scripts/custom/refine-smpl.py (:30-33, :74-84, :133-134, :187-208) over all F frames of a sequence, and its
 * gradient.  Definition: DESIGN.md section 4, "keypoint refinement".  In short, with the body model of ia_smpl_lbs_fwd:
 *   vert[f,v]  = T_v (vs + po) + transl[f],  T_v = sum_j w_vj A_j (A without the translation);  joint[f,j] = G_j.t + transl[f]
 *   points     [F,35,3]: the 24 joints, then the 11 vertices kp_vertex (nose, eyes, ears, toes and heels)
 *   uv[f,k]    = pinhole projection (proj [3,4], no guard on the depth) of model point M[k], k in BODY_25 order,
 *                M = 24 12 17 19 21 16 18 20 0 2 5 8 1 4 7 25 .. 34
 *   e[f,k]     = |keypoints[f,k].xy - uv[f,k]| where keypoints[f,k].conf > threshold (strict), else 0
 *   L_kp       = sum_{f, k != 8} e / (24 F);   L_t = sum_{f < F-1, v} |vert[f+1,v] - vert[f,v]| / ((F-1) V), absent for F == 1
 *   loss       [3] = L_kp + L_t, L_kp, L_t.   The gradient of a Euclidean norm at exactly zero is taken as zero.
 * fp32, fixed-order sums, no floating-point atomics: two calls on the same inputs give the same bits.
 *
 * ia_kp_workspace_bytes: scratch of either entry; 0 for n_frames < 1, n_verts < 1 or n_frames * n_verts * 3 >= 2^31.
 * ia_kp_loss_fwd: betas [10], pose [F,72], transl [F,3], proj [3,4], keypoints [F,25,3], kp_vertex [11] (device int32, each in
 *   [0, V)) -> verts [F,V,3], points [F,35,3], uv [F,25,2], loss [3]; each output may be NULL.
 * ia_kp_loss_bwd: the same inputs and verts as the forward wrote them -> d_betas [10], d_pose [F,72], d_transl [F,3] of loss[0];
 *   each may be NULL.  Nothing has to survive in ws from the forward call.                                                  */
#define IA_KP_N_POINTS 35
#define IA_KP_N_BODY25 25
#define IA_KP_N_VERTEX 11
size_t ia_kp_workspace_bytes(int n_frames, int n_verts);
int ia_kp_loss_fwd(const ia_smpl_body *body, const float *betas, const float *pose, const float *transl, int n_frames,
                   const float *proj, const float *keypoints, float threshold, const int32_t *kp_vertex, float *verts,
                   float *points, float *uv, float *loss, void *ws, size_t ws_bytes, void *stream);
int ia_kp_loss_bwd(const ia_smpl_body *body, const float *betas, const float *pose, const float *transl, int n_frames,
                   const float *proj, const float *keypoints, float threshold, const int32_t *kp_vertex, const float *verts,
                   float *d_betas, float *d_pose, float *d_transl, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_KEYPOINTS_H */
