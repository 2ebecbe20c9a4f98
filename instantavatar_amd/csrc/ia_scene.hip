// ia_scene.hip -- scene composition (no counterpart in the reference): several rendered avatars, a ground plane that receives their
// shadows and a background put into one frame.
//   the ground plane seen along the camera rays: hit, opacity, checker colour, hit point   (ia_scene_ground)
//   the shade of the ground points under the avatars' light-view opacity maps (PCF)        (ia_scene_shadow)
//   depth-ordered front-to-back compositing of K layers, the ground and a background       (ia_scene_composite)
//   zero-fill of the integer counter                                                       (ia_scene_zero)
//   the layers shaded by the shadows the avatars cast on each other and on themselves     (ia_scene_receive)
// The definition -- every formula and its order of operations -- is stated in include/instantavatar_hip_scene.h (ia_scene_receive:
// include/instantavatar_hip_scene_receive.h) and in DESIGN.md
// section 4 ("scene composition"); the library is built with -ffp-contract=off, so a fused multiply-add appears only where it is
// spelled.  Streaming kernels, one thread per pixel, no LDS; the layer planes are [K,R], so a wave reads 64 consecutive values of a
// plane.  Nothing here synchronises, allocates or reads on the host; no floating-point value is added atomically, so two calls give
// the same bytes.
//
// k_scene_composite<K>: the K + 1 contributors of a pixel (the ground is the last; one that does not take part becomes a no-op:
// key +inf, colour, opacity and depth term 0, which leave C, D and T bit-for-bit unchanged) are ordered by an insertion sort
// unrolled into compare-exchanges on registers -- no runtime-indexed array, no branch.
#include "ia_common.h"
#include "ia_mesh_dev.h"
#include "../../include/instantavatar_hip_scene.h"
#include "../../include/instantavatar_hip_scene_receive.h"

#define IA_SCENE_THREADS 256

namespace {

struct ScenePlane {          // the plane, the disc, the checker and the in-plane axes, all fp64
  double n[3], h, centre[3], r0, r1, cell, e1[3], e2[3];
  float g0[3], g1[3];
};

__device__ __forceinline__ bool scn_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }      // false for NaN

__global__ __launch_bounds__(IA_SCENE_THREADS) void k_scene_zero(int32_t *__restrict__ p, int n) {
  const int i = blockIdx.x * IA_SCENE_THREADS + threadIdx.x;
  if (i < n) p[i] = 0;
}

__global__ __launch_bounds__(IA_SCENE_THREADS) void k_scene_ground(const float *__restrict__ rays_o, const float *__restrict__ rays_d, int R,
                                                                   ScenePlane pl, float *__restrict__ t_g, float *__restrict__ a_g,
                                                                   float *__restrict__ c_g, float *__restrict__ P) {
  const int r = blockIdx.x * IA_SCENE_THREADS + threadIdx.x;
  if (r >= R) return;
  const size_t r3 = 3 * (size_t)r;
  const double o[3] = {rays_o[r3], rays_o[r3 + 1], rays_o[r3 + 2]}, d[3] = {rays_d[r3], rays_d[r3 + 1], rays_d[r3 + 2]};
  const double no = ia_dot3d(pl.n, o), nd = ia_dot3d(pl.n, d);
  const double t = (pl.h - no) / nd;
  const float tf = (float)t;
  float t_out = 0.f, a_out = 0.f, c_out[3] = {0.f, 0.f, 0.f}, p_out[3] = {0.f, 0.f, 0.f};
  if (no > pl.h && nd < 0.0 && scn_finite(tf) && tf > 0.f) {
    const double p[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
    const double q[3] = {p[0] - pl.centre[0], p[1] - pl.centre[1], p[2] - pl.centre[2]};
    const double rho = sqrt(ia_dot3d(q, q));
    const double a = rho <= pl.r0 ? 1.0 : (rho >= pl.r1 ? 0.0 : (pl.r1 - rho) / (pl.r1 - pl.r0));
    bool odd = false;
    if (pl.cell > 0.0) {
      double fu = floor(ia_dot3d(q, pl.e1) / pl.cell), fv = floor(ia_dot3d(q, pl.e2) / pl.cell);
      if (!(fabs(fu) < 4611686018427387904.0)) fu = 0.0;      // 2^62: beyond it a floor counts as 0 (also NaN)
      if (!(fabs(fv) < 4611686018427387904.0)) fv = 0.0;
      odd = (((long long)fu + (long long)fv) & 1ll) != 0;
    }
    t_out = tf;
    a_out = (float)a;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      c_out[ch] = odd ? pl.g1[ch] : pl.g0[ch];
      p_out[ch] = (float)p[ch];
    }
  }
  t_g[r] = t_out;
  a_g[r] = a_out;
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    c_g[r3 + ch] = c_out[ch];
    P[r3 + ch] = p_out[ch];
  }
}

// one bilinearly filtered tap of map m [S,S] at (x, y), both already clamped into [0, S - 1]
__device__ __forceinline__ float scn_tap(const float *__restrict__ m, int S, double x, double y) {
  const double xf = floor(x), yf = floor(y);
  const int i0 = (int)xf, j0 = (int)yf;
  const int i1 = min(i0 + 1, S - 1), j1 = min(j0 + 1, S - 1);
  const float fx = (float)(x - xf), fy = (float)(y - yf);
  const float m00 = m[(size_t)j0 * S + i0], m01 = m[(size_t)j0 * S + i1], m10 = m[(size_t)j1 * S + i0], m11 = m[(size_t)j1 * S + i1];
  const float top = __builtin_fmaf(fx, m01 - m00, m00), bot = __builtin_fmaf(fx, m11 - m10, m10);
  return __builtin_fmaf(fy, bot - top, top);
}

__global__ __launch_bounds__(IA_SCENE_THREADS) void k_scene_shadow(const float *__restrict__ P, const float *__restrict__ a_g, int R,
                                                                   const float *__restrict__ maps, const float *__restrict__ proj, int K,
                                                                   int S, int radius, float strength, double near,
                                                                   float *__restrict__ shade) {
  const int r = blockIdx.x * IA_SCENE_THREADS + threadIdx.x;
  if (r >= R) return;
  float sh = 1.f;
  if (a_g[r] != 0.f) {
    const size_t r3 = 3 * (size_t)r;
    const double p0 = P[r3], p1 = P[r3 + 1], p2 = P[r3 + 2];
    const double hi = (double)(S - 1), taps = (double)((2 * radius + 1) * (2 * radius + 1));
    for (int k = 0; k < K; k++) {
      const float *M = proj + 12 * (size_t)k;
      const double x0 = (((double)M[0] * p0 + (double)M[1] * p1) + (double)M[2] * p2) + (double)M[3];
      const double x1 = (((double)M[4] * p0 + (double)M[5] * p1) + (double)M[6] * p2) + (double)M[7];
      const double z = (((double)M[8] * p0 + (double)M[9] * p1) + (double)M[10] * p2) + (double)M[11];
      float abar = 0.f;
      if (z > near) {
        const double u = x0 / z, v = x1 / z;
        if (u >= 0.0 && u <= hi && v >= 0.0 && v <= hi) {           // NaN fails
          const float *m = maps + (size_t)k * S * S;
          double sum = 0.0;
          for (int dy = -radius; dy <= radius; dy++) {
            const double y = fmin(fmax(v + (double)dy, 0.0), hi);
            for (int dx = -radius; dx <= radius; dx++) {
              const double x = fmin(fmax(u + (double)dx, 0.0), hi);
              sum += (double)scn_tap(m, S, x, y);
            }
          }
          abar = (float)(sum / taps);
        }
      }
      sh = sh * (1.f - strength * abar);
    }
  }
  shade[r] = sh;
}

// contributor j of a pixel: ordered by (key, idx)
#define SCN_SWAP(x, i, j) \
  do {                    \
    const auto t__ = x[i]; \
    x[i] = lt ? x[j] : x[i]; \
    x[j] = lt ? t__ : x[j];  \
  } while (0)

template <int K>
__global__ __launch_bounds__(IA_SCENE_THREADS) void k_scene_composite(
    const float *__restrict__ c, const float *__restrict__ a, const float *__restrict__ d, int R, const float *__restrict__ t_g,
    const float *__restrict__ a_g, const float *__restrict__ c_g, const float *__restrict__ shade, const float *__restrict__ bg,
    int bg_const, float contact, float *__restrict__ rgb, float *__restrict__ alpha, float *__restrict__ depth,
    int32_t *__restrict__ contested) {
  constexpr int N = K + 1;
  const int r = blockIdx.x * IA_SCENE_THREADS + threadIdx.x;
  bool contest = false;
  if (r < R) {
    const size_t r3 = 3 * (size_t)r;
    float key[N], col0[N], col1[N], col2[N], op[N], term[N];
    int idx[N];
    bool ok[N];
#pragma unroll
    for (int k = 0; k < K; k++) {
      const size_t at = (size_t)k * R + r;
      const float ak = a[at], dk = d[at], c0 = c[3 * at], c1 = c[3 * at + 1], c2 = c[3 * at + 2];
      ok[k] = ak > 0.f && scn_finite(ak) && scn_finite(dk) && scn_finite(c0) && scn_finite(c1) && scn_finite(c2);
      key[k] = ok[k] ? dk / ak : __builtin_inff();
      col0[k] = ok[k] ? c0 : 0.f;
      col1[k] = ok[k] ? c1 : 0.f;
      col2[k] = ok[k] ? c2 : 0.f;
      op[k] = ok[k] ? ak : 0.f;
      term[k] = ok[k] ? dk : 0.f;
      idx[k] = k;
    }
    // pixels at which two opaque layers are closer than `contact` (on the unsorted layers)
#pragma unroll
    for (int i = 0; i < K; i++)
#pragma unroll
      for (int j = i + 1; j < K; j++)
        contest = contest || (ok[i] && ok[j] && op[i] >= 0.5f && op[j] >= 0.5f && __builtin_fabsf(key[i] - key[j]) < contact);
    {
      float tg = 0.f, ag = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f, sh = 0.f;
      if (t_g) {
        tg = t_g[r];
        ag = a_g[r];
        g0 = c_g[r3];
        g1 = c_g[r3 + 1];
        g2 = c_g[r3 + 2];
        sh = shade[r];
      }
      const bool okg = t_g && ag > 0.f && scn_finite(ag) && scn_finite(tg) && scn_finite(g0) && scn_finite(g1) && scn_finite(g2) &&
                       scn_finite(sh);
      ok[K] = okg;
      key[K] = okg ? tg : __builtin_inff();
      col0[K] = okg ? (g0 * sh) * ag : 0.f;
      col1[K] = okg ? (g1 * sh) * ag : 0.f;
      col2[K] = okg ? (g2 * sh) * ag : 0.f;
      op[K] = okg ? ag : 0.f;
      term[K] = okg ? ag * tg : 0.f;
      idx[K] = K;
    }
    // insertion sort as compare-exchanges of neighbours: after pass i the first i + 1 contributors are in order
#pragma unroll
    for (int i = 1; i < N; i++) {
#pragma unroll
      for (int j = i; j >= 1; j--) {
        const bool lt = key[j] < key[j - 1] || (key[j] == key[j - 1] && idx[j] < idx[j - 1]);
        SCN_SWAP(key, j - 1, j);
        SCN_SWAP(col0, j - 1, j);
        SCN_SWAP(col1, j - 1, j);
        SCN_SWAP(col2, j - 1, j);
        SCN_SWAP(op, j - 1, j);
        SCN_SWAP(term, j - 1, j);
        SCN_SWAP(idx, j - 1, j);
      }
    }
    float C0 = 0.f, C1 = 0.f, C2 = 0.f, D = 0.f, T = 1.f;
#pragma unroll
    for (int j = 0; j < N; j++) {
      C0 = C0 + T * col0[j];
      C1 = C1 + T * col1[j];
      C2 = C2 + T * col2[j];
      D = D + T * term[j];
      T = T * (1.f - op[j]);
    }
    float al = 1.f - T;
    if (bg) {
      const size_t b = bg_const ? 0 : r3;
      C0 = C0 + T * bg[b];
      C1 = C1 + T * bg[b + 1];
      C2 = C2 + T * bg[b + 2];
      al = 1.f;
    }
    rgb[r3] = C0;
    rgb[r3 + 1] = C1;
    rgb[r3 + 2] = C2;
    alpha[r] = al;
    depth[r] = D;
  }
  // one integer atomic per wave
  const unsigned long long b = __ballot(contest);
  if (ia_lane() == 0 && b) atomicAdd(contested, __popcll(b));
}

struct SceneLight {          // the light, the clauses and the facing ramp of k_scene_receive, all fp64 (the fp32 arguments converted)
  double L[3], near, bias_other, bias_self, cos0, dcos;      // dcos = cos1 - cos0
};

// k_scene_receive: one thread per pixel; layer j outside, caster k inside, so that nothing is indexed by a runtime k but global
// memory (no per-layer register arrays, no scratch).  A pixel none of whose K opacities is positive -- most of a frame -- copies its
// layers and leaves.  proj is read through a pointer indexed by k alone: wave-uniform, scalar loads.  The (2r + 1)^2 nearest taps of
// neighbouring pixels fall on neighbouring texels of maps that stay in L2; no LDS, no atomics.
__global__ __launch_bounds__(IA_SCENE_THREADS) void k_scene_receive(
    const float *__restrict__ rays_o, const float *__restrict__ rays_d, int R, const float *__restrict__ c, const float *__restrict__ a,
    const float *__restrict__ d, const float *__restrict__ nrm, const float *__restrict__ maps_a, const float *__restrict__ maps_d,
    const float *__restrict__ proj, int K, int S, int radius, float strength, SceneLight p, float *__restrict__ c_out,
    float *__restrict__ shade) {
  const int r = blockIdx.x * IA_SCENE_THREADS + threadIdx.x;
  if (r >= R) return;
  bool any = false;
  for (int k = 0; k < K; k++) any = any || a[(size_t)k * R + r] > 0.f;
  if (!any) {
    for (int k = 0; k < K; k++) {
      const size_t at = (size_t)k * R + r;
      shade[at] = 1.f;
      c_out[3 * at] = c[3 * at];
      c_out[3 * at + 1] = c[3 * at + 1];
      c_out[3 * at + 2] = c[3 * at + 2];
    }
    return;
  }
  const size_t r3 = 3 * (size_t)r;
  const double o[3] = {rays_o[r3], rays_o[r3 + 1], rays_o[r3 + 2]}, dir[3] = {rays_d[r3], rays_d[r3 + 1], rays_d[r3 + 2]};
  const double hi = (double)(S - 1), taps = (double)((2 * radius + 1) * (2 * radius + 1));
  const size_t SS = (size_t)S * S;
  for (int j = 0; j < K; j++) {
    const size_t at = (size_t)j * R + r;
    const float aj = a[at], dj = d[at], c0 = c[3 * at], c1 = c[3 * at + 1], c2 = c[3 * at + 2];
    const bool ok = aj > 0.f && scn_finite(aj) && scn_finite(dj) && scn_finite(c0) && scn_finite(c1) && scn_finite(c2);
    float sh = 1.f;
    if (ok) {
      const double z = (double)dj / (double)aj;
      const double X[3] = {o[0] + z * dir[0], o[1] + z * dir[1], o[2] + z * dir[2]};
      const double q[3] = {X[0] - p.L[0], X[1] - p.L[1], X[2] - p.L[2]};
      const double rho = sqrt(ia_dot3d(q, q));
      for (int k = 0; k < K; k++) {
        const float *M = proj + 12 * (size_t)k;
        const double x0 = (((double)M[0] * X[0] + (double)M[1] * X[1]) + (double)M[2] * X[2]) + (double)M[3];
        const double x1 = (((double)M[4] * X[0] + (double)M[5] * X[1]) + (double)M[6] * X[2]) + (double)M[7];
        const double zl = (((double)M[8] * X[0] + (double)M[9] * X[1]) + (double)M[10] * X[2]) + (double)M[11];
        float abar = 0.f;
        if (zl > p.near) {
          const double u = x0 / zl, v = x1 / zl;
          if (u >= 0.0 && u <= hi && v >= 0.0 && v <= hi) {           // NaN fails
            const float *ma = maps_a + (size_t)k * SS, *md = maps_d + (size_t)k * SS;
            const double reach = rho - (k == j ? p.bias_self : p.bias_other);
            double sum = 0.0;
            for (int dy = -radius; dy <= radius; dy++) {
              const size_t row = (size_t)(int)fmin(fmax(floor((v + (double)dy) + 0.5), 0.0), hi) * S;
              for (int dx = -radius; dx <= radius; dx++) {
                const size_t tap = row + (size_t)(int)fmin(fmax(floor((u + (double)dx) + 0.5), 0.0), hi);
                const float m = ma[tap], s = md[tap];
                const bool occludes = m > 0.f && (double)s < reach * (double)m;      // NaN: false
                sum += occludes ? (double)m : 0.0;
              }
            }
            abar = (float)(sum / taps);
          }
        }
        sh = sh * (1.f - strength * abar);
      }
      float g = 0.f;
      if (nrm) {
        const float n0 = nrm[3 * at], n1 = nrm[3 * at + 1], n2 = nrm[3 * at + 2];
        if ((n0 != 0.f || n1 != 0.f || n2 != 0.f) && scn_finite(n0) && scn_finite(n1) && scn_finite(n2)) {
          const double n[3] = {n0, n1, n2}, l[3] = {p.L[0] - X[0], p.L[1] - X[1], p.L[2] - X[2]};
          const double cosv = ia_dot3d(n, l) / sqrt(ia_dot3d(l, l));
          if (cosv == cosv) {
            const double t = (cosv - p.cos0) / p.dcos;
            g = (float)(1.0 - fmin(fmax(t, 0.0), 1.0));
          }
        }
      }
      sh = sh * (1.f - strength * g);
    }
    shade[at] = sh;
    c_out[3 * at] = ok ? c0 * sh : c0;
    c_out[3 * at + 1] = ok ? c1 * sh : c1;
    c_out[3 * at + 2] = ok ? c2 * sh : c2;
  }
}

inline bool scn_finite_h(double x) { return __builtin_isfinite(x); }

}  // namespace

extern "C" int ia_scene_zero(int32_t *words, int n, void *stream) {
  IA_CHECK_ARG(n >= 0, "ia_scene_zero: n = %d < 0", n);
  if (n == 0) return IA_OK;
  IA_CHECK_ARG(words, "ia_scene_zero: null pointer");
  IA_CHECK_ARG(((uintptr_t)words & 3) == 0, "ia_scene_zero: the words are not 4-byte aligned");
  hipLaunchKernelGGL(k_scene_zero, dim3(ia_div_up(n, IA_SCENE_THREADS)), dim3(IA_SCENE_THREADS), 0, (hipStream_t)stream, words, n);
  IA_LAUNCH_CHECK("k_scene_zero");
  return IA_OK;
}

extern "C" int ia_scene_ground(const float *rays_o, const float *rays_d, int R, float nx, float ny, float nz, float h, float g0r, float g0g,
                               float g0b, float g1r, float g1g, float g1b, float cell, float cx, float cy, float cz, float r0, float r1,
                               float *t_g, float *a_g, float *c_g, float *P, void *stream) {
  const char *who = "ia_scene_ground";
  IA_CHECK_ARG(R >= 0, "%s: R = %d < 0", who, R);
  const double n[3] = {(double)nx, (double)ny, (double)nz};
  const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  IA_CHECK_ARG(scn_finite_h(nn) && fabs(nn - 1.0) <= 1e-3, "%s: the normal (%g, %g, %g) has not unit length", who, n[0], n[1], n[2]);
  IA_CHECK_ARG(scn_finite_h(h), "%s: the offset h is not finite", who);
  IA_CHECK_ARG(scn_finite_h(g0r) && scn_finite_h(g0g) && scn_finite_h(g0b) && scn_finite_h(g1r) && scn_finite_h(g1g) && scn_finite_h(g1b),
               "%s: a colour is not finite", who);
  IA_CHECK_ARG(cell >= 0.f && scn_finite_h(cell), "%s: cell = %g must be finite and not negative", who, (double)cell);
  IA_CHECK_ARG(scn_finite_h(cx) && scn_finite_h(cy) && scn_finite_h(cz), "%s: the centre is not finite", who);
  IA_CHECK_ARG(r0 >= 0.f && r1 >= r0 && scn_finite_h(r1), "%s: the radii need 0 <= r0 = %g <= r1 = %g, finite", who, (double)r0, (double)r1);
  if (R == 0) return IA_OK;
  IA_CHECK_ARG(rays_o && rays_d && t_g && a_g && c_g && P, "%s: null pointer", who);
  ScenePlane pl;
  for (int i = 0; i < 3; i++) pl.n[i] = n[i];
  pl.h = (double)h;
  pl.centre[0] = (double)cx; pl.centre[1] = (double)cy; pl.centre[2] = (double)cz;
  pl.r0 = (double)r0; pl.r1 = (double)r1; pl.cell = (double)cell;
  pl.g0[0] = g0r; pl.g0[1] = g0g; pl.g0[2] = g0b;
  pl.g1[0] = g1r; pl.g1[1] = g1g; pl.g1[2] = g1b;
  // the in-plane axes: the coordinate axis least aligned with n, Gram-Schmidt, a cross product
  int ax = 0;
  for (int i = 1; i < 3; i++)
    if (fabs(n[i]) < fabs(n[ax])) ax = i;
  double s[3];
  for (int i = 0; i < 3; i++) s[i] = (i == ax ? 1.0 : 0.0) - n[ax] * n[i];
  const double len = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
  for (int i = 0; i < 3; i++) pl.e1[i] = s[i] / len;
  pl.e2[0] = n[1] * pl.e1[2] - n[2] * pl.e1[1];
  pl.e2[1] = n[2] * pl.e1[0] - n[0] * pl.e1[2];
  pl.e2[2] = n[0] * pl.e1[1] - n[1] * pl.e1[0];
  hipLaunchKernelGGL(k_scene_ground, dim3(ia_div_up(R, IA_SCENE_THREADS)), dim3(IA_SCENE_THREADS), 0, (hipStream_t)stream, rays_o, rays_d, R, pl, t_g, a_g,
                     c_g, P);
  IA_LAUNCH_CHECK("k_scene_ground");
  return IA_OK;
}

extern "C" int ia_scene_shadow(const float *P, const float *a_g, int R, const float *maps, const float *proj, int K, int S, int radius,
                               float strength, float near, float *shade, void *stream) {
  const char *who = "ia_scene_shadow";
  IA_CHECK_ARG(R >= 0, "%s: R = %d < 0", who, R);
  IA_CHECK_ARG(K >= 1 && K <= IA_SCENE_MAX_LAYERS, "%s: K = %d outside [1, %d]", who, K, IA_SCENE_MAX_LAYERS);
  IA_CHECK_ARG(S >= 1 && S <= IA_SCENE_MAX_MAP, "%s: S = %d outside [1, %d]", who, S, IA_SCENE_MAX_MAP);
  IA_CHECK_ARG(radius >= 0 && radius <= IA_SCENE_MAX_PCF, "%s: PCF radius %d outside [0, %d]", who, radius, IA_SCENE_MAX_PCF);
  IA_CHECK_ARG(strength >= 0.f && strength <= 1.f, "%s: strength = %g outside [0, 1]", who, (double)strength);
  IA_CHECK_ARG(near > 0.f && scn_finite_h(near), "%s: near must be positive and finite", who);
  if (R == 0) return IA_OK;
  IA_CHECK_ARG(P && a_g && maps && proj && shade, "%s: null pointer", who);
  hipLaunchKernelGGL(k_scene_shadow, dim3(ia_div_up(R, IA_SCENE_THREADS)), dim3(IA_SCENE_THREADS), 0, (hipStream_t)stream, P, a_g, R, maps, proj, K, S,
                     radius, strength, (double)near, shade);
  IA_LAUNCH_CHECK("k_scene_shadow");
  return IA_OK;
}

extern "C" int ia_scene_receive(const float *rays_o, const float *rays_d, int R, const float *c, const float *a, const float *d,
                                const float *nrm, const float *maps_a, const float *maps_d, const float *proj, int K, int S, float lx,
                                float ly, float lz, int radius, float strength, float near, float bias_other, float bias_self, float cos0,
                                float cos1, float *c_out, float *shade, void *stream) {
  const char *who = "ia_scene_receive";
  IA_CHECK_ARG(R >= 0, "%s: R = %d < 0", who, R);
  IA_CHECK_ARG(K >= 1 && K <= IA_SCENE_MAX_LAYERS, "%s: K = %d outside [1, %d]", who, K, IA_SCENE_MAX_LAYERS);
  IA_CHECK_ARG(S >= 1 && S <= IA_SCENE_MAX_MAP, "%s: S = %d outside [1, %d]", who, S, IA_SCENE_MAX_MAP);
  IA_CHECK_ARG(radius >= 0 && radius <= IA_SCENE_MAX_PCF, "%s: PCF radius %d outside [0, %d]", who, radius, IA_SCENE_MAX_PCF);
  IA_CHECK_ARG(strength >= 0.f && strength <= 1.f, "%s: strength = %g outside [0, 1]", who, (double)strength);
  IA_CHECK_ARG(near > 0.f && scn_finite_h(near), "%s: near must be positive and finite", who);
  IA_CHECK_ARG(bias_other >= 0.f && scn_finite_h(bias_other) && bias_self >= 0.f && scn_finite_h(bias_self),
               "%s: the biases (%g, %g) must be finite and not negative", who, (double)bias_other, (double)bias_self);
  IA_CHECK_ARG(cos0 >= -1.f && cos0 < cos1 && cos1 <= 1.f, "%s: the facing ramp needs -1 <= cos0 = %g < cos1 = %g <= 1", who, (double)cos0,
               (double)cos1);
  IA_CHECK_ARG(scn_finite_h(lx) && scn_finite_h(ly) && scn_finite_h(lz), "%s: the light is not finite", who);
  if (R == 0) return IA_OK;
  IA_CHECK_ARG(rays_o && rays_d && c && a && d && maps_a && maps_d && proj && c_out && shade, "%s: null pointer", who);
  SceneLight p;
  p.L[0] = (double)lx; p.L[1] = (double)ly; p.L[2] = (double)lz;
  p.near = (double)near; p.bias_other = (double)bias_other; p.bias_self = (double)bias_self;
  p.cos0 = (double)cos0; p.dcos = (double)cos1 - (double)cos0;
  hipLaunchKernelGGL(k_scene_receive, dim3(ia_div_up(R, IA_SCENE_THREADS)), dim3(IA_SCENE_THREADS), 0, (hipStream_t)stream, rays_o, rays_d, R, c, a, d,
                     nrm, maps_a, maps_d, proj, K, S, radius, strength, p, c_out, shade);
  IA_LAUNCH_CHECK("k_scene_receive");
  return IA_OK;
}

extern "C" int ia_scene_composite(const float *c, const float *a, const float *d, int K, int R, const float *t_g, const float *a_g,
                                  const float *c_g, const float *shade, const float *bg, int bg_const, float contact, float *rgb,
                                  float *alpha, float *depth, int32_t *contested, void *stream) {
  const char *who = "ia_scene_composite";
  IA_CHECK_ARG(K >= 1 && K <= IA_SCENE_MAX_LAYERS, "%s: K = %d outside [1, %d]", who, K, IA_SCENE_MAX_LAYERS);
  IA_CHECK_ARG(R >= 0, "%s: R = %d < 0", who, R);
  IA_CHECK_ARG(contact >= 0.f && scn_finite_h(contact), "%s: contact = %g must be finite and not negative", who, (double)contact);
  const int ng = (t_g != nullptr) + (a_g != nullptr) + (c_g != nullptr) + (shade != nullptr);
  IA_CHECK_ARG(ng == 0 || ng == 4, "%s: the ground needs t_g, a_g, c_g and shade, or none of them", who);
  if (R == 0) return IA_OK;
  IA_CHECK_ARG(c && a && d && rgb && alpha && depth && contested, "%s: null pointer", who);
  const dim3 grid(ia_div_up(R, IA_SCENE_THREADS)), block(IA_SCENE_THREADS);
  hipStream_t s = (hipStream_t)stream;
#define SCN_LAUNCH(KK)                                                                                                              \
  case KK:                                                                                                                          \
    hipLaunchKernelGGL(k_scene_composite<KK>, grid, block, 0, s, c, a, d, R, t_g, a_g, c_g, shade, bg, bg_const, contact, rgb, alpha, \
                       depth, contested);                                                                                           \
    break
  switch (K) {
    SCN_LAUNCH(1);
    SCN_LAUNCH(2);
    SCN_LAUNCH(3);
    SCN_LAUNCH(4);
    SCN_LAUNCH(5);
    SCN_LAUNCH(6);
    SCN_LAUNCH(7);
    SCN_LAUNCH(8);
  }
#undef SCN_LAUNCH
  IA_LAUNCH_CHECK("k_scene_composite");
  return IA_OK;
}
