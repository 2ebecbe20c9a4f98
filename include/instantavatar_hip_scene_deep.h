/*
 * instantavatar_hip_scene_deep.h -- exact scene compositing where avatars interleave along a ray: the entry point of
 * csrc/ia_scene_deep.hip.  Conventions, constants and "fp32" exactly as instantavatar_hip_scene.h defines them (device pointers,
 * `stream` as void*, no synchronisation, no allocation, 0 = IA_OK; no fused multiply-add unless written as fma).  A header of its
 * own, bound by `_lib` as a table of its own.  Definition: below, restated in DESIGN.md section 4, "scene composition", step 5.  It
 * lifts LIMIT (layered compositing) of instantavatar_hip_scene.h for the camera view: instead of one colour, opacity and depth per
 * avatar and pixel, every SAMPLE of every avatar along the pixel's ray is composited in depth order.  Two calls with the same inputs
 * give the same bytes: nothing is accumulated across threads but one integer count.
 */
#ifndef INSTANTAVATAR_HIP_SCENE_DEEP_H
#define INSTANTAVATAR_HIP_SCENE_DEEP_H

#include "instantavatar_hip_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IA_SCENE_DEEP_MAX_SLOTS 1024

/* ia_scene_deep_composite: n pixels, K lists of S slots each, 1 <= K <= IA_SCENE_MAX_LAYERS, 1 <= S <= IA_SCENE_DEEP_MAX_SLOTS,
 *   n >= 0 (n = 0: IA_OK, nothing is launched).  z, delta, sigma [K,S,n] and rgb [K,S,n,3]: slot-major planes, pixels fastest -- slot
 *   s of list k of pixel p is at (k S + s) n + p.  The slots of a list are the ones the avatar's own test render visits along the
 *   pixel's ray, in its order (ia_raymarch_test / ia_composite_test): a filled prefix, delta <= 0 (or NaN) marks an empty slot; z is
 *   the parameter along the pixel's world ray, the same for every avatar.  factor: NULL, or [K,n] a colour factor per list and
 *   pixel (the shade a layer receives).  t_g, a_g, c_g, shade [n], [n], [n,3], [n]: the ground as ia_scene_composite takes it, all
 *   four or all NULL.  bg: NULL, [3] (bg_const != 0) or [n,3].  thresh >= 0, finite: the opacity below which a sample is skipped
 *   (0.01f in the renderer).  One thread per pixel; all fp32 in the order written.
 *   State: C = (0, 0, 0), D = 0, T = 1; per list a cursor s_k = 0 and the list's OWN transmittance T_k = 1.
 *   The ground takes part iff t_g != NULL, a_g > 0 and a_g, t_g, c_g (3), shade are all finite (ia_scene_composite's rule); it is
 *   pending until it has been consumed.
 *   Repeat, at most K S + 1 times (every step consumes a slot or the ground):
 *     1. head of list k: exists iff s_k < S, delta > 0, z is finite and (double)T_k > 1e-4 -- the conditions under which the
 *        avatar's own compositor goes on, so a list ends where the avatar's own render would have stopped.
 *     2. the next item is the head with the smallest (z, k); the pending ground competes with (t_g, K): an exact tie goes to the
 *        lower list and the ground comes last.  No head and no pending ground: the loop ends.
 *     3. a sample: sg = sigma, c = rgb of the slot, each replaced by 0 when not finite; dl = delta, z = z of the slot.
 *        tau = __expf(-sg * dl), alpha = 1 - tau; the cursor advances.
 *        alpha < thresh: the sample is skipped, nothing else changes.
 *        otherwise: c = c * f_k per channel when factor != NULL; w = alpha * T; C = C + w * c per channel; D = D + w * z;
 *        T = T * tau; T_k = T_k * tau.
 *     4. the ground: C = C + T * ((c_g * shade) * a_g) per channel; D = D + T * (a_g * t_g); T = T * (1 - a_g).
 *   There is no joint early stop: the lists are already cut by their own stops.
 *   End: rgb_out = C + T * bg per channel and alpha_out = 1 with a background; rgb_out = C and alpha_out = 1 - T without;
 *   depth_out = D.
 *   Interleaved pixels.  Take the owners (k, or K for the ground) of the items that were composited (not skipped), in merged order,
 *   with consecutive repeats removed; the pixel is interleaved iff a list appears twice in that sequence.  (The ground ends a run,
 *   so a ground between two samples of one avatar makes the pixel interleaved: there the layered order is not the merged one.)
 *   *interleaved (device int32, accumulated; the caller zeroes it with ia_scene_zero) += the number of interleaved pixels; one
 *   integer atomic per wave.
 *   K = 1 without factor, ground and background gives the bytes ia_composite_test leaves in (color, depth_out, nohit) started from
 *   (0, 0, 1) -- on finite inputs -- with alpha_out = 1 - nohit.  Where no pixel is interleaved the merged order is the layered
 *   order, and both compositors evaluate the same real-number expression.
 *   On a bad argument the status is returned and nothing is written.                                                          */
int ia_scene_deep_composite(const float *z, const float *delta, const float *sigma, const float *rgb, int K, int S, int n,
                            const float *factor, const float *t_g, const float *a_g, const float *c_g, const float *shade, const float *bg,
                            int bg_const, float thresh, float *rgb_out, float *alpha_out, float *depth_out, int32_t *interleaved,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_SCENE_DEEP_H */
