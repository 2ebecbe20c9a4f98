// ia_scene_deep.hip -- exact scene compositing where avatars interleave along a ray (no counterpart in the reference): the K sample
// lists of a pixel, one per avatar and each exactly the slots its own test render visits, are merged by depth and composited front to
// back together with the ground and the background                                                          (ia_scene_deep_composite)
// The definition -- every formula and its order of operations -- is stated in include/instantavatar_hip_scene_deep.h and in DESIGN.md
// section 4 ("scene composition", step 5); the library is built with -ffp-contract=off.
//
// k_scene_deep<K>: one thread per pixel, no LDS.  The planes are slot-major [K,S,n], pixels fastest: neighbouring pixels have
// neighbouring cursors, so a wave's load of one plane touches a few 256-byte runs.  Per list the thread keeps the head's key and
// step, the cursor and the list's own transmittance in registers; K is a template parameter and every loop over the lists is
// unrolled, so that the minimum is a compare chain and the chosen list advances through an `if (k == sel)` ladder -- nothing is
// indexed by a runtime k, no scratch.  The merge loop is bounded by K S + 1: every step consumes a slot or the ground.  Nothing
// synchronises or allocates; no floating-point value is added atomically, so two calls give the same bytes; the one counter is added
// once per wave from a ballot.
#include "ia_common.h"
#include "../../include/instantavatar_hip_scene_deep.h"

#define IA_DEEP_THREADS 256

namespace {

__device__ __forceinline__ bool deep_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }      // false for NaN

// the head of a list at cursor s: its key (+inf: the list has ended) and its step
__device__ __forceinline__ void deep_head(const float *__restrict__ z, const float *__restrict__ delta, size_t list, int s, int S,
                                          size_t n, float Tk, float &key, float &dl) {
  key = __builtin_inff();
  dl = 0.f;
  if (s < S && (double)Tk > 1e-4) {
    const size_t at = list + (size_t)s * n;
    const float d = delta[at], zz = z[at];
    if (d > 0.f && deep_finite(zz)) {
      key = zz;
      dl = d;
    }
  }
}

template <int K>
__global__ __launch_bounds__(IA_DEEP_THREADS) void k_scene_deep(
    const float *__restrict__ z, const float *__restrict__ delta, const float *__restrict__ sigma, const float *__restrict__ rgb, int S,
    int n_, const float *__restrict__ factor, const float *__restrict__ t_g, const float *__restrict__ a_g, const float *__restrict__ c_g,
    const float *__restrict__ shade, const float *__restrict__ bg, int bg_const, float thresh, float *__restrict__ rgb_out,
    float *__restrict__ alpha_out, float *__restrict__ depth_out, int32_t *__restrict__ interleaved) {
  const int p = blockIdx.x * IA_DEEP_THREADS + threadIdx.x;
  const size_t n = (size_t)n_;
  bool inter = false;
  if (p < n_) {
    const size_t p3 = 3 * (size_t)p;
    float key[K], hdl[K], Tk[K], fk[K];
    int cur[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
      cur[k] = 0;
      Tk[k] = 1.f;
      fk[k] = factor ? factor[(size_t)k * n + p] : 1.f;
      deep_head(z, delta, (size_t)k * S * n + p, 0, S, n, 1.f, key[k], hdl[k]);
    }
    // the ground: pending while it takes part and has not been consumed
    float tg = 0.f, ag = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f;
    bool ground = false;
    if (t_g) {
      tg = t_g[p];
      ag = a_g[p];
      const float sh = shade[p];
      g0 = c_g[p3];
      g1 = c_g[p3 + 1];
      g2 = c_g[p3 + 2];
      ground = ag > 0.f && deep_finite(ag) && deep_finite(tg) && deep_finite(g0) && deep_finite(g1) && deep_finite(g2) && deep_finite(sh);
      g0 = (g0 * sh) * ag;
      g1 = (g1 * sh) * ag;
      g2 = (g2 * sh) * ag;
    }
    float C0 = 0.f, C1 = 0.f, C2 = 0.f, D = 0.f, T = 1.f;
    int last = -1;
    unsigned seen = 0u;
    const int steps = K * S + 1;
    for (int it = 0; it < steps; it++) {
      int sel = -1;
      float zmin = __builtin_inff();
#pragma unroll
      for (int k = 0; k < K; k++)
        if (key[k] < zmin) {      // strict: a tie goes to the lower layer
          zmin = key[k];
          sel = k;
        }
      if (ground && !(zmin <= tg)) {      // the ground comes last among equals
        C0 = C0 + T * g0;
        C1 = C1 + T * g1;
        C2 = C2 + T * g2;
        D = D + T * (ag * tg);
        T = T * (1.f - ag);
        ground = false;
        last = K;      // the ground ends a run of owners
        continue;
      }
      if (sel < 0) break;
#pragma unroll
      for (int k = 0; k < K; k++)
        if (k == sel) {
          const size_t list = (size_t)k * S * n + p;
          const size_t at = list + (size_t)cur[k] * n;
          float sg = sigma[at], c0 = rgb[3 * at], c1 = rgb[3 * at + 1], c2 = rgb[3 * at + 2];
          sg = deep_finite(sg) ? sg : 0.f;
          c0 = deep_finite(c0) ? c0 : 0.f;
          c1 = deep_finite(c1) ? c1 : 0.f;
          c2 = deep_finite(c2) ? c2 : 0.f;
          const float tau = __expf(-sg * hdl[k]);
          const float alpha = 1.0f - tau;
          cur[k]++;
          if (!(alpha < thresh)) {
            if (factor) {
              c0 = c0 * fk[k];
              c1 = c1 * fk[k];
              c2 = c2 * fk[k];
            }
            const float w = alpha * T;
            C0 = C0 + w * c0;
            C1 = C1 + w * c1;
            C2 = C2 + w * c2;
            D = D + w * key[k];
            T = T * tau;
            Tk[k] = Tk[k] * tau;
            if (last != k) {
              inter = inter || ((seen >> k) & 1u);
              seen |= 1u << k;
              last = k;
            }
          }
          deep_head(z, delta, list, cur[k], S, n, Tk[k], key[k], hdl[k]);
        }
    }
    float al = 1.f - T;
    if (bg) {
      const size_t b = bg_const ? 0 : p3;
      C0 = C0 + T * bg[b];
      C1 = C1 + T * bg[b + 1];
      C2 = C2 + T * bg[b + 2];
      al = 1.f;
    }
    rgb_out[p3] = C0;
    rgb_out[p3 + 1] = C1;
    rgb_out[p3 + 2] = C2;
    alpha_out[p] = al;
    depth_out[p] = D;
  }
  // one integer atomic per wave
  const unsigned long long b = __ballot(inter);
  if (ia_lane() == 0 && b) atomicAdd(interleaved, __popcll(b));
}

}  // namespace

extern "C" int ia_scene_deep_composite(const float *z, const float *delta, const float *sigma, const float *rgb, int K, int S, int n,
                                       const float *factor, const float *t_g, const float *a_g, const float *c_g, const float *shade,
                                       const float *bg, int bg_const, float thresh, float *rgb_out, float *alpha_out, float *depth_out,
                                       int32_t *interleaved, void *stream) {
  const char *who = "ia_scene_deep_composite";
  IA_CHECK_ARG(K >= 1 && K <= IA_SCENE_MAX_LAYERS, "%s: K = %d outside [1, %d]", who, K, IA_SCENE_MAX_LAYERS);
  IA_CHECK_ARG(S >= 1 && S <= IA_SCENE_DEEP_MAX_SLOTS, "%s: S = %d outside [1, %d]", who, S, IA_SCENE_DEEP_MAX_SLOTS);
  IA_CHECK_ARG(n >= 0, "%s: n = %d < 0", who, n);
  IA_CHECK_ARG(thresh >= 0.f && __builtin_isfinite(thresh), "%s: thresh = %g must be finite and not negative", who, (double)thresh);
  const int ng = (t_g != nullptr) + (a_g != nullptr) + (c_g != nullptr) + (shade != nullptr);
  IA_CHECK_ARG(ng == 0 || ng == 4, "%s: the ground needs t_g, a_g, c_g and shade, or none of them", who);
  if (n == 0) return IA_OK;
  IA_CHECK_ARG(z && delta && sigma && rgb && rgb_out && alpha_out && depth_out && interleaved, "%s: null pointer", who);
  const dim3 grid(ia_div_up(n, IA_DEEP_THREADS)), block(IA_DEEP_THREADS);
  hipStream_t s = (hipStream_t)stream;
#define DEEP_LAUNCH(KK)                                                                                                               \
  case KK:                                                                                                                            \
    hipLaunchKernelGGL(k_scene_deep<KK>, grid, block, 0, s, z, delta, sigma, rgb, S, n, factor, t_g, a_g, c_g, shade, bg, bg_const, \
                       thresh, rgb_out, alpha_out, depth_out, interleaved);                                                           \
    break
  switch (K) {
    DEEP_LAUNCH(1);
    DEEP_LAUNCH(2);
    DEEP_LAUNCH(3);
    DEEP_LAUNCH(4);
    DEEP_LAUNCH(5);
    DEEP_LAUNCH(6);
    DEEP_LAUNCH(7);
    DEEP_LAUNCH(8);
  }
#undef DEEP_LAUNCH
  IA_LAUNCH_CHECK("k_scene_deep");
  return IA_OK;
}
