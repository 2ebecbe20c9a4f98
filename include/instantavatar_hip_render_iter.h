/*
 * instantavatar_hip_render_iter.h -- the four kernels of ia_render_test's wave-front loop (csrc/ia_render.hip), each alone on
 * caller-owned device buffers.  Called by tests/ only (tests/test_gpu_render_iter_kernels.py), like the ia_selftest_* entries
 * of instantavatar_hip.h.  Conventions as there: device pointers, `stream` as void*, no synchronisation, no allocation,
 * 0 = IA_OK, errors through ia_last_error.  A header of its own, bound by `_lib` as a table of its own: the table of
 * instantavatar_hip.h is pinned to its prototypes.
 */
#ifndef INSTANTAVATAR_HIP_RENDER_ITER_H
#define INSTANTAVATAR_HIP_RENDER_ITER_H

#include "instantavatar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every entry makes the launch ia_render_test makes (same grid of ceil(R / 256) workgroups, same block, same template
 * choice: the marcher reads the bit grid from LDS when G == 64 and occ_bits is 16-byte aligned, from memory otherwise).
 * `state` points to consecutive iteration records of EIGHT int32 each:
 *     [0] n_alive    rays handed to this iteration (at most R)      [4] iters   earlier iterations that had rays
 *     [1] n_samples  compact sample counter of this iteration       [5] n_step  N_step of this iteration   } written by
 *     [2] n_cand     compact candidate counter                      [6] n_eff   rays actually processed    } the marcher
 *     [3] k_before   samples-per-ray budget consumed before it      [7] pad
 *   ia_render_init_rays:         near_w = near, step = (far - near) / max_samples, colour / depth / counter 0, nohit 1,
 *                                alive = 0 .. R-1; zeroes 1024 records behind `state` and sets record 0's n_alive = R.
 *   ia_render_march_compact:     works on record state[0] (the caller fills n_alive and k_before, n_samples must be 0) and
 *                                writes n_step, n_eff, n_samples there and k_before, iters of record state[1]; n_eff rays of
 *                                `alive` are marched for n_step samples each: ray_off / ray_cnt per alive SLOT, s_pts / s_t
 *                                compact (samples at or past sample_cap are counted, not stored), near_w and counter per ray.
 *                                occ_bits as ia_occupancy_pack writes it (the tail words are read), 4-byte aligned.
 *   ia_render_composite_compact: composites the samples of record state[0] (n_eff, n_step as the marcher left them) with the
 *                                maximum over each sample's candidates (pt_off / pt_cnt into cand_rgb / cand_sigma, invalid
 *                                slots 0, non-finite -> 0) into colour / depth / nohit, appends the surviving rays to alive_next
 *                                and counts them into record state[1]'s n_alive.
 *   ia_render_finalize:          rgb = colour + nohit * bg (NULL: white), depth, alpha = 1 - nohit, counter; n_alive_out
 *                                (NULL or int32[2]) = {state_end's n_alive, or 0 when its k_before >= max_samples; its iters}.   */
int ia_render_init_rays(int R, const float *near, const float *far, float *near_w, float *step, float *color, float *depth,
                        float *nohit, float *counter, int32_t *alive, int max_samples, int32_t *state, void *stream);
int ia_render_march_compact(const float *rays_o, const float *rays_d, float *near_w, const float *far, const float *step,
                            const int32_t *alive, int R, const uint32_t *occ_bits, int G, const float *aabb, int32_t *state,
                            float *s_pts, float *s_t, int32_t *ray_off, int32_t *ray_cnt, float *counter, int sample_cap,
                            int max_samples, int max_batch, void *stream);
int ia_render_composite_compact(const int32_t *alive, int32_t *alive_next, int32_t *state, const int32_t *ray_off,
                                const int32_t *ray_cnt, const float *s_t, const float *step, const int32_t *pt_off,
                                const uint8_t *pt_cnt, const float *cand_rgb, const float *cand_sigma, int n_init, int R,
                                float *color, float *depth, float *nohit, float thresh, void *stream);
int ia_render_finalize(int R, const float *color, const float *depth, const float *nohit, const float *counter, const float *bg,
                       const int32_t *state_end, int max_samples, int32_t *n_alive_out, float *rgb, float *depth_out, float *alpha,
                       float *counter_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* INSTANTAVATAR_HIP_RENDER_ITER_H */
