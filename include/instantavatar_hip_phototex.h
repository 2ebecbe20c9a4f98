/*
 * instantavatar_hip_phototex.h -- photo-texture entry points of libinstantavatar_hip.so (csrc/ia_phototex.hip): the frames of a
 * sequence projected back onto the texture atlas of a mesh.  Conventions as in instantavatar_hip.h (device pointers, `stream` as
 * void*, no synchronisation, no allocation, 0 = IA_OK); a header of its own, bound by `_lib` as a table of its own.  Definition:
 * DESIGN.md section 4, "photo texture".  The atlas layout (B, T, owner, the weights u0, u1, u2 of a texel, gutter texels included) is
 * the one of instantavatar_hip_texture.h; the camera is the rasteriser's (instantavatar_hip_raster.h).
 *
 * Per texel g and frame f, in fp64 on the fp32 inputs: p = u0 a_f + u1 b_f + u2 c_f on the posed corners of the owner face, n its unit
 * normal (b_f - a_f) x (c_f - a_f); x = R p + t, (u, v) = (fx x.x / x.z + cx, fy x.y / x.z + cy); c = -(R n) . x / |x|.  The frame
 * contributes iff the face is valid in it (indices inside [0, nv), finite corners, a normal that is finite and not zero), x.z >= near,
 * c > cos_min, 0 <= u < W - 1 and 0 <= v < H - 1 (all four pixels (i0 + {0,1}, j0 + {0,1}), i0 = floor(u), j0 = floor(v), inside the
 * image) and every one of the four has mask >= 0.5, depth > 0 and |x.z - depth| <= depth_tol.  Then rgb = the bilinear filter of the
 * four uint8 pixels / 255 with the weights u - i0, v - j0, w = c^power, and S += w rgb, W += w, seen += 1, frames in ascending order.
 */
#ifndef INSTANTAVATAR_HIP_PHOTOTEX_H
#define INSTANTAVATAR_HIP_PHOTOTEX_H

#include "instantavatar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IA_PHOTOTEX_MAX_FRAMES 65536
#define IA_PHOTOTEX_MAX_DIM 16384
#define IA_PHOTOTEX_ACC_STRIDE 40

/* ia_phototex_acc_bytes (host only): the size of the accumulator of `count` texels, IA_PHOTOTEX_ACC_STRIDE bytes each (S [3] and W
 *   as fp64, seen as int32, 4 bytes unused); 0 for count < 0.  The record of texel k of a range starts at byte k * the stride, so
 *   the accumulator of a sub-range is a pointer into the accumulator of the range; 8-byte aligned.
 * ia_phototex_zero: zero-fills the records of `count` texels (a kernel).                                                       */
size_t ia_phototex_acc_bytes(int count);
int ia_phototex_zero(void *acc, int count, void *stream);

/* ia_phototex_accumulate: adds F >= 1 frames to the records of the texels first .. first + count of the atlas (row-major, texel g =
 *   y T + x; acc is the accumulator OF THAT RANGE: record 0 belongs to texel `first`).  verts [F,nv,3] posed vertices, faces [nf,3],
 *   T = ia_tex_atlas_size(nf, B); w2c [F,4,4]; fx, fy, cx, cy, near > 0 shared by the F frames; images [F,H,W,3] uint8, masks
 *   [F,H,W] fp32 (NULL: every pixel passes), depth [F,H,W] fp32 (camera z of the posed mesh, 0 = empty).  0 <= cos_min < 1,
 *   power >= 0, depth_tol >= 0, all finite.  The sums continue from what the records hold, one frame after the other, so the bytes
 *   do not depend on how the frames are split into calls or the texels into ranges.                                            */
int ia_phototex_accumulate(const float *verts, int nv, const int32_t *faces, int nf, int B, int T, int first, int count, int F,
                           const float *w2c, float fx, float fy, float cx, float cy, float near, const uint8_t *images,
                           const float *masks, const float *depth, int H, int W, float cos_min, float power, float depth_tol, void *acc,
                           void *stream);

/* ia_phototex_resolve: for the `count` texels of acc: seen [count] = the record's count; atlas [count,3] = 0 where owner [count] < 0,
 *   fp32(S / W) where seen >= min_frames (>= 1), else the texel of base [count,3] (NULL: 0).  *unseen (device int32, ACCUMULATED: the
 *   caller zeroes it) counts the owned texels with seen == 0.                                                                   */
int ia_phototex_resolve(const void *acc, const float *base, const int32_t *owner, int count, int min_frames, float *atlas, int32_t *seen,
                        int32_t *unseen, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_PHOTOTEX_H */
