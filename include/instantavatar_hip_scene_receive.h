/*
 * instantavatar_hip_scene_receive.h -- the avatars of a composed scene receive shadows, each other's and their own: one more entry
 * point of csrc/ia_scene.hip.  Conventions, constants and "fp64" / "fp32" / dot exactly as instantavatar_hip_scene.h defines them
 * (device pointers, `stream` as void*, no synchronisation, no allocation, 0 = IA_OK; no fused multiply-add unless written as fma).
 * A header of its own, bound by `_lib` as a table of its own: the table of instantavatar_hip_scene.h is pinned to its four
 * functions.  Definition: below, restated in DESIGN.md section 4, "scene composition".  Two calls with the same inputs give the same
 * bytes: nothing is accumulated across threads.
 */
#ifndef INSTANTAVATAR_HIP_SCENE_RECEIVE_H
#define INSTANTAVATAR_HIP_SCENE_RECEIVE_H

#include "instantavatar_hip_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ia_scene_receive: the layers c, a, d [K,R,3], [K,R], [K,R] of ia_scene_composite shaded by the shadows the avatars cast on each
 *   other and on themselves: c_out [K,R,3] = the shaded layers (given to ia_scene_composite in place of c), shade [K,R] = their
 *   multipliers.  rays_o, rays_d [R,3]: the rays the layers were rendered along (unit directions; the depth sums count metres along
 *   them).  nrm: NULL, or [K,R,3] the surface normals of the layers in the rays' frame (`render_image_fast(normals=True)`: unit
 *   length, or zero where a pixel has none).  maps_a, maps_d [K,S,S]: avatar k rendered from the light with projection proj [K,3,4]
 *   (as ia_scene_shadow) -- its opacity and its depth SUM along the light's unit-length rays (NOT divided by the opacity).
 *   L = (lx, ly, lz): the point light in the rays' frame, finite.  radius: the PCF radius r in 0 .. IA_SCENE_MAX_PCF;
 *   0 <= strength <= 1; near > 0; 1 <= S <= IA_SCENE_MAX_MAP; 1 <= K <= IA_SCENE_MAX_LAYERS; R >= 0; bias_other, bias_self >= 0,
 *   finite: metres by which a caster must lie nearer to the light than the receiver, for another avatar and for the receiver's
 *   own; -1 <= cos0 < cos1 <= 1: the facing ramp.  One thread per pixel; per pixel and layer j:
 *   the layer receives iff a_j > 0 and c_j (3), a_j, d_j are all finite (it "takes part" in ia_scene_composite).  A layer that does
 *   not receive gets shade = 1 and c_out = c bit for bit (NaNs included).
 *   Receiver, fp64: z = d_j / a_j, X = o + z dir (per component), q = X - L, rho = sqrt(dot(q, q)).
 *   Caster k = 0 .. K - 1 in layer order (k = j included), fp64: x_i = ((M_i0 X_0 + M_i1 X_1) + M_i2 X_2) + M_i3 with M = proj_k,
 *   zl = x_2, u = x_0 / zl, v = x_1 / zl.  abar_jk = 0 when not (zl > near), or when not (0 <= u <= S - 1 and 0 <= v <= S - 1)
 *   (NaN: 0).  Otherwise, for dy = -r .. r (outer) and dx = -r .. r (inner), NEAREST taps (a depth is not interpolated across a
 *   silhouette): xi = min(max(floor((u + dx) + 0.5), 0), S - 1), yi = min(max(floor((v + dy) + 0.5), 0), S - 1),
 *   m = maps_a[k,yi,xi], s = maps_d[k,yi,xi].  The tap occludes iff m > 0 and s < (rho - bias) * m, compared in fp64, with
 *   bias = bias_self when k == j and bias_other otherwise (NaN: not occluding; the tap's mean depth s / m lies nearer to the light
 *   than the receiver by more than the bias, written without the division).  The tap's value is m when it occludes, else 0; the
 *   values are summed in that order in fp64 and abar_jk = fp32(sum / (2r + 1)^2).
 *   Facing term, fp64, with n = nrm[j]: l = L - X, cosv = dot(n, l) / sqrt(dot(l, l)), t = (cosv - cos0) / (cos1 - cos0),
 *   f = min(max(t, 0), 1), g = fp32(1 - f).  g = 0 instead when nrm == NULL, when n is zero or not finite, or when cosv is NaN.
 *   (A surface that faces away from the light lies in its own attached shadow; there the light-view depth would decide by noise.)
 *   fp32, from shade = 1: shade = shade * (1 - strength * abar_jk) over k in layer order, then shade = shade * (1 - strength * g);
 *   c_out = c_j * shade per channel (premultiplied colour: the shaded layer).  The product form is ia_scene_shadow's.
 *   On a bad argument the status is returned and nothing is written.                                                          */
int ia_scene_receive(const float *rays_o, const float *rays_d, int R, const float *c, const float *a, const float *d, const float *nrm,
                     const float *maps_a, const float *maps_d, const float *proj, int K, int S, float lx, float ly, float lz, int radius,
                     float strength, float near, float bias_other, float bias_self, float cos0, float cos1, float *c_out, float *shade,
                     void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_SCENE_RECEIVE_H */
