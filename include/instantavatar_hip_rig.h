/*
 * instantavatar_hip_rig.h -- rigged-export entry points of libinstantavatar_hip.so (csrc/ia_rig.hip): per-vertex joint indices and
 * weights sampled from the skinning-weight volume, the bone matrices / joint quaternions / root translations of a whole pose track,
 * and linear-blend skinning of a mesh over all frames of the track in one launch.  Conventions as in instantavatar_hip.h (device
 * pointers, `stream` as void*, no synchronisation, no allocation, 0 = IA_OK); a header of its own, bound by `_lib` as a table of its
 * own.  Definitions: DESIGN.md section 4, "rigged export".
 */
#ifndef INSTANTAVATAR_HIP_RIG_H
#define INSTANTAVATAR_HIP_RIG_H

#include "instantavatar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IA_RIG_MAX_INFLUENCES 24   /* = IA_N_JOINTS: a rig with all of them reproduces the transform grid's skinning */

/* ia_rig_weights: the skinning weights of n canonical points xc [n,3].
 *   full [n,24] fp32 (may be NULL) = the trilinear sample of voxel_w at the point, align_corners, border padding: what
 *     ForwardDeformer.query_weights returns and ia_snarf_inverse_skinning gathers.  voxel_w is [24,D,H,W], or [D,H,W,24] with
 *     channel_last != 0 (16-byte aligned then).
 *   joints [n,K] uint8, weights [n,K] fp32, 1 <= K <= 24: the K largest of them in descending order, a tie going to the lower joint
 *     index (a NaN weight is never selected), divided by their fp32 sum taken in slot order.  A slot whose weight is exactly 0 names
 *     joint 0.  A point with a non-finite coordinate, or whose kept weights sum to 0 or to a non-finite value, gets joint 0 with
 *     weight 1 in slot 0 and (0, 0) in the others; `full` of a point with a non-finite coordinate is zero.                        */
int ia_rig_weights(const float *xc, int n, const float *voxel_w, int channel_last, const ia_snarf_grid *grid, int K, uint8_t *joints,
                   float *weights, float *full, void *stream);

/* ia_rig_track: F frames of a pose track, one workgroup per frame.  joints_rest [24,3], parents [24], tfs_inv_t [24,4,4] as for
 *   ia_smpl_tfs; poses [F,72] axis-angle, transl [F,3] (may be NULL: 0).
 *   bones [F,24,4,4]  = A_j . tfs_inv_t_j with A = ia_smpl_tfs's `A` of the frame (transl folded in): the world-frame transform of a
 *                       canonical point by joint j.  The fourth row is written as (0, 0, 0, 1).
 *   quat [F,24,4]     = the joints' local rotations as unit quaternions x, y, z, w: ang = |theta + 1e-8|, dir = theta / ang,
 *                       q = normalise(dir sin(ang / 2), cos(ang / 2))  (may be NULL)
 *   root_t [F,3]      = J_0 + transl: the root node's local translation  (may be NULL)                                          */
int ia_rig_track(const float *joints_rest, const int32_t *parents, const float *poses, const float *transl, const float *tfs_inv_t,
                 int F, float *bones, float *quat, float *root_t, void *stream);

/* ia_rig_skin: linear-blend skinning of n vertices over F frames.  joints [n,K] uint8 (values above 23 are read as 23), weights
 *   [n,K] fp32, 1 <= K <= 24; bones [F,24,4,4] (rows 0..2 are read; 16-byte aligned).  Per frame and vertex
 *     M = sum_k w_k bones[f][j_k]  (12 entries, each accumulated with fmaf from 0 in slot order)
 *     out_verts [F,n,3]   = M [x; 1]             (per row fmaf(M2, z, fmaf(M1, y, M0 x)) + M3)
 *     out_normals [F,n,3] = normalise(M_3x3 n)   (the zero vector where the product is zero or not finite) -- what a glTF viewer
 *                           computes, not the inverse transpose.  normals and out_normals are given together or both NULL.      */
int ia_rig_skin(const float *verts, const float *normals, int n, const uint8_t *joints, const float *weights, int K, const float *bones,
                int F, float *out_verts, float *out_normals, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_RIG_H */
