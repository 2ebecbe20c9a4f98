/*
 * instantavatar_hip_overlay.h -- looking at a custom sequence: the per-pixel work of overlaying the posed body, the mask outline and
 * the 2D skeleton on a batch of frames, and the pixel counts of the silhouette IoU (csrc/ia_overlay.hip; what scripts/visualize-SMPL.py
 * of the reference shows through aitviewer and an OpenGL context).  Conventions as in instantavatar_hip_masks.h (device pointers,
 * `stream` as void* and never NULL here, no allocation, scratch through `ws`, 0 = IA_OK, no host synchronisation); a header of its
 * own, bound by `_lib` as a ninth table.
 *
 * Definitions ("sequence inspection").  Everything but the shade factor of ia_overlay_face_shade is integer
 * arithmetic.  Frames are independent; two calls, or the same frame at another position of a batch, give the same bytes.  Every entry
 * refuses n, H, W < 1, n > IA_OVERLAY_MAX_FRAMES, a parameter out of its range and a NULL required pointer with IA_ERR_ARG and then
 * writes nothing.  Nothing has to be zeroed by the caller.
 *
 * ia_overlay_blend: images [n,H,W,3] uint8, layer [n,H,W,4] uint8 (r, g, b, alpha), opacity in [0, 256] -> out [n,H,W,3] uint8; out may BE
 *   images (the same pointer), not overlap it otherwise.  Per pixel with the layer's alpha byte A:
 *       a = (opacity * A + 127) / 255          (integer division; 0 .. 256)
 *       out_c = (img_c * (256 - a) + layer_c * a + 128) >> 8
 *   so opacity 0 or A = 0 copies the image and opacity 256 with A = 255 gives the layer.  Every element of out is written.
 *
 * ia_overlay_outline: masks [n,H,W] uint8, thickness t in [1, IA_OVERLAY_MAX_THICKNESS], colour r, g, b in [0, 255]; in place on images
 *   [n,H,W,3].  A pixel is outline iff mask > 0 and some pixel OF THE IMAGE within Chebyshev distance t has mask == 0.  Positions outside
 *   the image do not count: a mask cut by the image border gets no line there.  Outline pixels take the colour; no other byte of images
 *   is written.
 *
 * ia_overlay_face_shade: face_id [H,W] int32 (-1 = empty, as ia_raster_resolve writes it), verts [nv,3] fp32, faces [nf,3] int32, w2c
 *   [4,4] fp32 row-major, tint r, g, b in [0, 255] -> layer [H,W,4] uint8 (4-byte aligned).  Per covered pixel, with d1 = R (v1 - v0), d2 =
 *   R (v2 - v0) (R = the upper-left 3 x 3 of w2c) and c = d1 x d2:  s = 0.25 + 0.75 |c_z| / |c|, colour byte floor(tint s + 0.5), alpha 255.
 *   A degenerate face (|c| = 0, or not finite) gives s = 0.25.  An empty pixel gives four zero bytes, and so does a face id outside
 *   [0, nf) or a face with a vertex index outside [0, nv): neither is dereferenced.  Flat shading from face ids: a gather, no
 *   floating-point scatter, so the layer is a function of its inputs only.
 *
 * ia_overlay_skeleton: points [n,K,3] fp32 (x, y, confidence), 1 <= K <= IA_OVERLAY_MAX_POINTS; segments [S,2] int32 and segment_rgb [S,3]
 *   uint8, 0 <= S <= IA_OVERLAY_MAX_SEGMENTS (both may be NULL when S = 0); the discs' colour point_r, point_g, point_b; threshold;
 *   half_width_q in [1, 64] and radius_q in [0, 128], both in QUARTER pixels; in place on images [n,H,W,3], H, W <= 32768.  Exact integer geometry:
 *       a coordinate is quantised q = floor(4 x + 0.5) (exact in fp32 for |x| <= 32768); pixel (px, py) has its centre at (4 px, 4 py)
 *       a point is valid iff x, y and confidence are finite, confidence > threshold (equal is not drawn) and |x|, |y| <= 32768
 *       segment (i, j) is drawn iff both indices are in [0, K) and both points are valid; otherwise it is skipped, not dereferenced.
 *         With a, b its quantised ends, p the pixel centre, d = b - a, e = p - a, L2 = d . d, t = d . e:
 *           L2 == 0 or t <= 0   inside iff e . e <= hw^2
 *           t >= L2             inside iff |p - b|^2 <= hw^2
 *           otherwise           inside iff (d_x e_y - d_y e_x)^2 <= hw^2 L2      (compared exactly, see ia_overlay.hip)
 *       the disc of a valid point k covers p iff |p - q_k|^2 <= radius_q^2
 *   A pixel takes point_rgb if a disc covers it, else the colour of the HIGHEST-index segment that covers it, else it is not written
 *   (all discs share one colour, so "the highest-index disc" and "any disc" are the same picture).  A gather: no races.
 *
 * ia_overlay_stats_workspace_bytes: scratch of ia_overlay_stats; 0 outside 1 <= n <= IA_OVERLAY_MAX_FRAMES, H, W >= 1, H * W < 2^31.
 * ia_overlay_stats: a, b [n,H,W] uint8 (a torch bool tensor's bytes are valid input) -> out [n,4] int32: the pixels of a frame with
 *   a > 0 and b > 0, with a > 0 or b > 0, with a > 0, with b > 0.  Integer sums in two stages (partial sums per workgroup in ws, then one
 *   wave per frame): independent of scheduling. */
#ifndef INSTANTAVATAR_HIP_OVERLAY_H
#define INSTANTAVATAR_HIP_OVERLAY_H

#include "instantavatar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IA_OVERLAY_MAX_FRAMES 65535
#define IA_OVERLAY_MAX_THICKNESS 8
#define IA_OVERLAY_MAX_POINTS 64
#define IA_OVERLAY_MAX_SEGMENTS 64
int ia_overlay_blend(const uint8_t *images, const uint8_t *layer, int n, int H, int W, int opacity, uint8_t *out, void *stream);
int ia_overlay_outline(const uint8_t *masks, int n, int H, int W, int thickness, int r, int g, int b, uint8_t *images, void *stream);
int ia_overlay_face_shade(const int32_t *face_id, int H, int W, const float *verts, int nv, const int32_t *faces, int nf, const float *w2c,
                          int r, int g, int b, uint8_t *layer, void *stream);
int ia_overlay_skeleton(const float *points, int n, int K, const int32_t *segments, const uint8_t *segment_rgb, int S, int point_r,
                        int point_g, int point_b, float threshold, int half_width_q, int radius_q, int H, int W, uint8_t *images,
                        void *stream);
size_t ia_overlay_stats_workspace_bytes(int n, int H, int W);
int ia_overlay_stats(const uint8_t *a, const uint8_t *b, int n, int H, int W, int32_t *out, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_OVERLAY_H */
