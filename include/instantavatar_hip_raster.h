/*
 * instantavatar_hip_raster.h -- the triangle-rasteriser entry points of libinstantavatar_hip.so (csrc/ia_raster.hip).
 * Conventions as in instantavatar_hip.h (device pointers, `stream` as void*, no synchronisation, no allocation, scratch
 * through `ws`, 0 = IA_OK); a header of its own, bound by `_lib` as a table of its own next to the other four.
 */
#ifndef INSTANTAVATAR_HIP_RASTER_H
#define INSTANTAVATAR_HIP_RASTER_H

#include "instantavatar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- a deterministic triangle rasteriser with a z-buffer (no counterpart in the reference, whose mesh pictures come from
 * aitviewer and pytorch3d).  Definition: DESIGN.md section 4, "rasteriser".  In short:
 *   camera      OpenCV pinhole (x right, y down, z forward): p = R X + t with R, t from a DEVICE w2c [4,4]; u = fx p.x / p.z + cx,
 *               v = fy p.y / p.z + cy; pixel (x, y) is sampled AT (x, y), no half-pixel offset -- the ray of drivers/animate.make_rays
 *               through pixel (x, y) is K^-1 [x, y, 1], so a raster frame overlays a volumetric frame of the same camera.
 *   projection  xy [nv,2] int32 = rint(256 u), rint(256 v) (8 sub-pixel bits), inv_z [nv] = 1 / p.z, evaluated in fp64 and rounded
 *               once.  A vertex is INVALID when p.z < near, when a coordinate is not finite, or when |xy| > 2^22 on either axis:
 *               inv_z = 0 (and xy = 0).  2^22 keeps every edge function inside int64: coordinate differences stay below 2^24, a
 *               product below 2^48, an edge function below 2^49.  A face with an invalid vertex is skipped; nothing is clipped.
 *   coverage    exact integers.  A = (x1-x0)(y2-y0) - (x2-x0)(y1-y0); A == 0: skipped; front-facing iff A < 0 (A is the z component
 *               of (b-a) x (c-a) on the screen, and the outward normal of a face seen from outside points at the camera, towards
 *               -z); cull != 0 skips back faces.  s = sign(A), P = (256 x, 256 y), E = s ((xb-xa)(Py-ya) - (yb-ya)(Px-xa)) for the
 *               edges v1->v2, v2->v0, v0->v1; covered iff every E > 0, or E == 0 on a top-left edge (dy < 0, or dy == 0 && dx > 0,
 *               with dx = s (xb-xa), dy = s (yb-ya)).
 *   visibility  l_i = fp32(E_i) / fp32(|A|), iz = fma(l_2, w_c, fma(l_1, w_b, l_0 w_a)) in fp32 (w = inv_z), key =
 *               (uint64(bits(iz)) << 32) | (0xFFFFFFFF - face), combined with a 64-bit atomic max: the nearest fragment wins, an
 *               exact tie goes to the smaller face index, and the result does not depend on scheduling.  0 = empty.
 *   resolve     face_id (-1 = empty), depth = 1 / iz (0 = empty), C perspective-correct channels sum(l_i w_i a_i) / iz (0 = empty).
 * Limits: 0 <= nv, nf < 2^31, 1 <= H, W <= IA_RASTER_MAX_DIM, 0 <= C <= IA_RASTER_MAX_CHANNELS; anything else is an argument error.
 *
 * ia_raster_workspace_bytes: the scratch of ia_raster_visibility (counters + the queue of large faces); 0 for arguments outside
 *   the limits.
 * ia_raster_project: xy / inv_z of nv vertices [nv,3]; near > 0.
 * ia_raster_visibility: zero-fills vis [H*W] (a kernel) and rasterises the nf faces [nf,3] into it.  A vertex counts as invalid
 *   when its inv_z is not a positive finite number or its |xy| exceeds 2^22 (hand-made input is held to the projection's promise);
 *   so does a vertex index outside [0, nv).  ws is read again by ia_raster_resolve.
 * ia_raster_resolve: per pixel face_id [H*W], depth [H*W] and, with C > 0, attr_out [H*W,C] interpolated from attrs [nv,C] (both
 *   may be NULL when C == 0); counts (device, 2 x int32) = faces skipped by ia_raster_visibility (invalid vertex, A == 0, or
 *   culled), covered pixels.  xy / inv_z / faces / ws as given to ia_raster_visibility.                                       */
#define IA_RASTER_MAX_DIM 16384
#define IA_RASTER_MAX_CHANNELS 8
size_t ia_raster_workspace_bytes(int nv, int nf, int H, int W);
int ia_raster_project(const float *verts, int nv, const float *w2c, float fx, float fy, float cx, float cy, float near,
                      int32_t *xy, float *inv_z, void *stream);
int ia_raster_visibility(const int32_t *xy, const float *inv_z, int nv, const int32_t *faces, int nf, int H, int W, int cull,
                         int64_t *vis, void *ws, size_t ws_bytes, void *stream);
int ia_raster_resolve(const int32_t *xy, const float *inv_z, int nv, const int32_t *faces, int nf, const int64_t *vis, int H, int W,
                      const float *attrs, int C, const void *ws, size_t ws_bytes, int32_t *face_id, float *depth, float *attr_out,
                      int32_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_RASTER_H */
