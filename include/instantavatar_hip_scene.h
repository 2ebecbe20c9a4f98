/*
 * instantavatar_hip_scene.h -- scene-composition entry points of libinstantavatar_hip.so (csrc/ia_scene.hip): several rendered
 * avatars, a ground plane that receives their shadows and a background put into one frame.  Conventions as in instantavatar_hip.h
 * (device pointers, `stream` as void*, no synchronisation, no allocation, 0 = IA_OK); a header of its own, bound by `_lib` as a table
 * of its own.  Definition: DESIGN.md section 4, "scene composition".  One thread per pixel, R = H W pixels, K layers,
 * 1 <= K <= IA_SCENE_MAX_LAYERS.  Two calls with the same inputs give the same bytes: nothing here adds floating-point values
 * atomically (the one atomic adds an integer count).
 *
 * Arithmetic.  "fp64" below means: the fp32 inputs converted to double, every operation a separate IEEE double operation in the
 * order written (no fused multiply-add), one rounding to fp32 where the result is stored.  "fp32" means separate IEEE single
 * operations in the order written; a fused multiply-add appears only where it is written as fma(a, b, c) = a b + c.
 * dot(a, b) = (a0 b0 + a1 b1) + a2 b2.
 *
 * LIMIT (layered compositing).  A layer is a whole rendered avatar reduced to one colour, one opacity and one depth per pixel, and
 * the layers of a pixel are composited in the order of their depths.  That is exact only where the supports of the avatars along
 * the ray do not interleave (one is entirely in front of the other); where two bodies intertwine along a ray the nearer one is
 * put entirely in front.  `contested` of ia_scene_composite counts the pixels at which that may have happened.
 * ia_scene_deep_composite (instantavatar_hip_scene_deep.h) lifts this limit for the camera view: it composites every sample of every
 * avatar in depth order; the light views below keep it.
 * LIMIT (shadows).  The ground receives the avatars' shadows (ia_scene_shadow); the avatars receive each other's and their own only
 * when ia_scene_receive is run on the layers before they are composited, and then as a multiplier on colours that already carry
 * the lighting the avatar was captured under: one point light, no colour, nothing falls onto the background.  A receiver is one
 * point per pixel and layer, the layer's expected depth, so LIMIT (layered compositing) holds for shadows as well.
 */
#ifndef INSTANTAVATAR_HIP_SCENE_H
#define INSTANTAVATAR_HIP_SCENE_H

#include "instantavatar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IA_SCENE_MAX_LAYERS 8
#define IA_SCENE_MAX_PCF 3
#define IA_SCENE_MAX_MAP 8192

/* ia_scene_zero: words [n] int32 = 0 (a kernel; the counter of ia_scene_composite is zeroed with it).  n >= 0.               */
int ia_scene_zero(int32_t *words, int n, void *stream);

/* ia_scene_ground: the plane n . x = h seen along the rays rays_o, rays_d [R,3].  n = (nx, ny, nz) has unit length (|n|^2 within
 *   1e-3 of 1) and points to the side objects stand on.  g0, g1: the two colours; cell >= 0: the edge of a checker cell (0: plain
 *   g0); centre (cx, cy, cz): the centre of the disc and the origin of the checker; 0 <= r0 <= r1: the disc is opaque inside r0
 *   and gone outside r1.  All finite.
 *   In-plane axes, computed once in fp64 on the host from the fp32 n: i = the index of the smallest |n_i| (the lowest index among
 *   equals), e = the i-th coordinate axis, s = e - n_i n, e1 = s / sqrt(dot(s, s)), e2 = n x e1
 *   = (n1 e1_2 - n2 e1_1, n2 e1_0 - n0 e1_2, n0 e1_1 - n1 e1_0).
 *   Per pixel, fp64: no = dot(n, o), nd = dot(n, d), t = (h - no) / nd, p = o + t d (per component), q = p - centre,
 *   rho = sqrt(dot(q, q)), a = 1 if rho <= r0, else 0 if rho >= r1, else (r1 - rho) / (r1 - r0); u = dot(q, e1), v = dot(q, e2),
 *   parity = (floor(u / cell) + floor(v / cell)) & 1 on 64-bit integers (0 when cell == 0; a floor that is not below 2^62 in
 *   magnitude counts as 0); colour = g1 if parity else g0.
 *   The pixel hits iff no > h and nd < 0 and fp32(t) is finite and > 0.  Then t_g [R] = fp32(t), a_g [R] = fp32(a) (multiplied by
 *   nothing else), c_g [R,3] = the colour (unshadowed), P [R,3] = fp32(p); otherwise all of them are 0.                         */
int ia_scene_ground(const float *rays_o, const float *rays_d, int R, float nx, float ny, float nz, float h, float g0r, float g0g, float g0b,
                    float g1r, float g1g, float g1b, float cell, float cx, float cy, float cz, float r0, float r1, float *t_g, float *a_g,
                    float *c_g, float *P, void *stream);

/* ia_scene_shadow: shade [R] of the ground points P [R,3] with opacity a_g [R] under K lights' opacity maps.  maps [K,S,S] fp32:
 *   map k is the opacity (alpha) of avatar k rendered from the light with projection proj [K,3,4] = K_light [R | t] (pixel centres
 *   at integers, as `raster.Camera`; the last row of K_light is 0 0 1, so the third component is the camera depth).  radius: the PCF
 *   radius r in 0 .. IA_SCENE_MAX_PCF; 0 <= strength <= 1; near > 0; 1 <= S <= IA_SCENE_MAX_MAP.
 *   Per pixel with a_g != 0 and layer k, fp64: x_i = ((M_i0 P_0 + M_i1 P_1) + M_i2 P_2) + M_i3, z = x_2, u = x_0 / z, v = x_1 / z.
 *   The layer contributes abar_k = 0 when not (z > near), or when not (0 <= u <= S - 1 and 0 <= v <= S - 1) (NaN: 0).  Otherwise,
 *   for dy = -r .. r (outer) and dx = -r .. r (inner): x = min(max(u + dx, 0), S - 1), i0 = floor(x), i1 = min(i0 + 1, S - 1),
 *   fx = fp32(x - i0); the same for y = v + dy with j0, j1, fy (clamp to the edge); in fp32, the lerp form of ia_tex_sample:
 *   top = fma(fx, m[j0,i1] - m[j0,i0], m[j0,i0]), bot = fma(fx, m[j1,i1] - m[j1,i0], m[j1,i0]), tap = fma(fy, bot - top, top); the
 *   taps are summed in that order in fp64 and abar_k = fp32(sum / (2r + 1)^2).
 *   shade = product over k in layer order, in fp32 starting from 1: shade = shade * (1 - strength * abar_k).  A pixel with
 *   a_g == 0 gets shade = 1.                                                                                                   */
int ia_scene_shadow(const float *P, const float *a_g, int R, const float *maps, const float *proj, int K, int S, int radius,
                    float strength, float near, float *shade, void *stream);

/* ia_scene_composite: K layers, optionally the ground, optionally a background -> one frame.  c [K,R,3]: premultiplied colour (sum
 *   of w c over the samples of a ray), a [K,R]: opacity (1 - T), d [K,R]: depth SUM (sum of w t, NOT divided by the opacity) -- what
 *   `render_image_fast` returns when the batch carries a zero `bg_color`.  t_g, a_g, c_g, shade: the ground (ia_scene_ground,
 *   ia_scene_shadow), all four given or all four NULL.  bg: NULL, or [R,3] (bg_const == 0), or one colour [3] (bg_const != 0).
 *   contact >= 0.  Per pixel, fp32:
 *   layer k takes part iff a_k > 0 and c_k (3), a_k, d_k are all finite; its key is z_k = d_k / a_k, its colour c_k, its opacity
 *   a_k, its depth term d_k, its index k.  The ground takes part iff a_g > 0 and t_g, a_g, c_g (3), shade are all finite; its key is
 *   t_g, its colour (c_g * shade) * a_g, its opacity a_g, its depth term a_g * t_g, its index K (an exact tie of keys goes to the
 *   avatar).  The contributors are ordered by (key, index) ascending and composited front to back from C = 0, D = 0, T = 1:
 *   C = C + T * colour (per channel), D = D + T * term, T = T * (1 - opacity).
 *   rgb [R,3] = C + T * bg (C without a background), alpha [R] = 1 with a background, 1 - T without, depth [R] = D.
 *   *contested (device int32, ACCUMULATED: the caller zeroes it, ia_scene_zero) counts the pixels at which two layers i < j that
 *   take part both have a >= 0.5 and |z_i - z_j| < contact: there the layered order may be wrong (LIMIT above).                 */
int ia_scene_composite(const float *c, const float *a, const float *d, int K, int R, const float *t_g, const float *a_g, const float *c_g,
                       const float *shade, const float *bg, int bg_const, float contact, float *rgb, float *alpha, float *depth,
                       int32_t *contested, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_SCENE_H */
