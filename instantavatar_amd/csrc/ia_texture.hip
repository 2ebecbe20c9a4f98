// ia_texture.hip -- a texture atlas over a triangle mesh (no counterpart in the reference): every face owns half of a square block
// of texels, so nothing is unwrapped and no seam needs dilating.
//   corner coordinates of every face in the atlas                          (ia_tex_corner_uv)
//   the surface point, face normal and owner of a range of texels          (ia_tex_texel_points)
//   the nearest level crossing along the normal from K density samples     (ia_tex_snap)
//   bilinear filtering of the atlas at interpolated coordinates            (ia_tex_sample)
// The definitions are stated in DESIGN.md section 4 ("texture atlas") and in include/instantavatar_hip_texture.h.  Streaming
// kernels: one thread per texel, corner or pixel, consecutive threads on consecutive addresses, no LDS.  Nothing here synchronises,
// allocates or reads on the host; the only atomic adds integers, so two calls on the same input give the same bytes.
// The layout of the atlas (which half and face own a texel, the texel's weights) and the face pieces are ia_mesh_dev.h's.
#include "ia_common.h"
#include "ia_mesh_dev.h"
#include "../../include/instantavatar_hip_texture.h"

#define IA_TEX_THREADS 256

namespace {

// blocks per atlas row: max(1, ceil(sqrt(ceil(nf / 2)))) in integers
inline int tex_blocks_per_row(int nf) {
  const long long nq = ((long long)nf + 1) / 2;
  long long nb = 1;
  while (nb * nb < nq) nb++;
  return (int)nb;
}

// the local texel (x, y) of corner k of the face in half h
__device__ __forceinline__ void tex_corner(int B, int h, int k, int &x, int &y) {
  const int L = B - 3;
  x = k == 1 ? L : 0;
  y = k == 2 ? L : 0;
  if (h) {
    x = B - 1 - x;
    y = B - 1 - y;
  }
}

__global__ __launch_bounds__(IA_TEX_THREADS) void k_tex_corner_uv(int nf, int B, int nb, float *__restrict__ uv) {
  const int i = blockIdx.x * IA_TEX_THREADS + threadIdx.x;      // one (face, corner) per thread: 3 nf <= 3 * 2^25
  if (i >= 3 * nf) return;
  const int f = i / 3, k = i - 3 * f;
  const int q = f >> 1;
  int x, y;
  tex_corner(B, f & 1, k, x, y);
  uv[2 * (size_t)i] = (float)((q % nb) * B + x) + 0.5f;
  uv[2 * (size_t)i + 1] = (float)((q / nb) * B + y) + 0.5f;
}

__global__ __launch_bounds__(IA_TEX_THREADS) void k_tex_texel_points(const float *__restrict__ verts, int nv,
                                                                     const int32_t *__restrict__ faces, int nf, int B, int T, int first,
                                                                     int count, const float *__restrict__ t, float t_scalar,
                                                                     float *__restrict__ pts, float *__restrict__ normal,
                                                                     int32_t *__restrict__ owner) {
  const int idx = blockIdx.x * IA_TEX_THREADS + threadIdx.x;
  if (idx >= count) return;
  const int g = first + idx;                                     // < T^2 <= 2^28
  const int y = g / T, x = g - y * T;
  const int bc = x / B, br = y / B;
  int i = x - bc * B, j = y - br * B;
  const int h = ia_atlas_half(B, i, j);
  int f = ia_atlas_face(br, bc, T / B, h);
  double pt[3] = {0, 0, 0}, n[3] = {0, 0, 0};
  if (f >= nf) f = -1;
  if (f >= 0) {
    int v[3];
    double p[3][3];
    ia_face_load(faces, f, v);
    bool ok = ia_face_in_range(v, nv);
    if (ok) {
      ia_face_corners(verts, v, p);
      ok = ia_corners_finite(p);
    }
    if (!ok) {
      f = -1;
    } else {
      double u[3], m[3];
      ia_atlas_weights(B, i, j, u);
      ia_face_point(p, u, pt);
      ia_face_cross(p, m);
      const double len = ia_len3d(m);
      if (len > 0.0 && __builtin_isfinite(len)) {
#pragma unroll
        for (int d = 0; d < 3; d++) n[d] = m[d] / len;
      }
      const double tt = (double)t_scalar + (t ? (double)t[idx] : 0.0);
#pragma unroll
      for (int d = 0; d < 3; d++) pt[d] += tt * n[d];
    }
  }
#pragma unroll
  for (int d = 0; d < 3; d++) {
    pts[3 * (size_t)idx + d] = (float)pt[d];
    if (normal) normal[3 * (size_t)idx + d] = (float)n[d];
  }
  if (owner) owner[idx] = f;
}

__global__ __launch_bounds__(IA_TEX_THREADS) void k_tex_snap(const float *__restrict__ sigma, int K, int n, float level, float dist,
                                                             const int32_t *__restrict__ owner, float *__restrict__ t_out,
                                                             int32_t *__restrict__ unsnapped) {
  const int i = blockIdx.x * IA_TEX_THREADS + threadIdx.x;
  bool miss = false;
  if (i < n) {
    float best = 0.f;
    if (dist > 0.f && (!owner || owner[i] >= 0)) {
      const float h = (2.f * dist) / (float)(K - 1);
      const int mid = (K - 1) / 2;
      bool found = false;
      float s0 = sigma[i] - level;
      for (int k = 0; k + 1 < K; k++) {
        const float s1 = sigma[(size_t)(k + 1) * n + i] - level;
        if (__builtin_isfinite(s0) && __builtin_isfinite(s1) && ((s0 >= 0.f) != (s1 >= 0.f))) {
          const float tk = (float)(k - mid) * h;
          const float r = tk + h * (s0 / (s0 - s1));
          if (!found || fabsf(r) < fabsf(best)) best = r;       // strict: a tie keeps the smaller k
          found = true;
        }
        s0 = s1;
      }
      if (!found) best = 0.f;
      miss = !found;
    }
    t_out[i] = best;
  }
  // one integer atomic per wave
  const unsigned long long b = __ballot(miss);
  if (ia_lane() == 0 && b) atomicAdd(unsnapped, __popcll(b));
}

__device__ __forceinline__ float tex_lerp(float w, float a, float b) { return __builtin_fmaf(w, b - a, a); }

__global__ __launch_bounds__(IA_TEX_THREADS) void k_tex_sample(const float *__restrict__ atlas, int T, const float *__restrict__ uv,
                                                               const float *__restrict__ mask, int R, float *__restrict__ out) {
  const int r = blockIdx.x * IA_TEX_THREADS + threadIdx.x;
  if (r >= R) return;
  const float u = uv[2 * (size_t)r], v = uv[2 * (size_t)r + 1];
  float c0 = 0.f, c1 = 0.f, c2 = 0.f;
  if ((!mask || mask[r] != 0.f) && __builtin_isfinite(u) && __builtin_isfinite(v)) {
    const float top = (float)(T - 1);
    const float x = fminf(fmaxf(u - 0.5f, 0.f), top), y = fminf(fmaxf(v - 0.5f, 0.f), top);
    const float xf = floorf(x), yf = floorf(y);
    const int i0 = (int)xf, j0 = (int)yf;                       // in [0, T-1] after the clamp
    const int i1 = min(i0 + 1, T - 1), j1 = min(j0 + 1, T - 1);
    const float fx = x - xf, fy = y - yf;
    const float *r0 = atlas + (size_t)j0 * T * 3, *r1 = atlas + (size_t)j1 * T * 3;
    const float *p00 = r0 + 3 * (size_t)i0, *p01 = r0 + 3 * (size_t)i1, *p10 = r1 + 3 * (size_t)i0, *p11 = r1 + 3 * (size_t)i1;
    c0 = tex_lerp(fy, tex_lerp(fx, p00[0], p01[0]), tex_lerp(fx, p10[0], p11[0]));
    c1 = tex_lerp(fy, tex_lerp(fx, p00[1], p01[1]), tex_lerp(fx, p10[1], p11[1]));
    c2 = tex_lerp(fy, tex_lerp(fx, p00[2], p01[2]), tex_lerp(fx, p10[2], p11[2]));
  }
  out[3 * (size_t)r] = c0;
  out[3 * (size_t)r + 1] = c1;
  out[3 * (size_t)r + 2] = c2;
}

}  // namespace

extern "C" int ia_tex_atlas_size(int nf, int B) {
  if (nf < 0 || B < IA_TEX_MIN_BLOCK || B > IA_TEX_MAX_BLOCK) return 0;
  const long long T = (long long)tex_blocks_per_row(nf) * B;
  return T <= IA_TEX_MAX_SIZE ? (int)T : 0;
}

// the layout arguments shared by two entry points
static int tex_check_layout(const char *who, int nf, int B, int T) {
  IA_CHECK_ARG(nf >= 0, "%s: nf = %d < 0", who, nf);
  IA_CHECK_ARG(B >= IA_TEX_MIN_BLOCK && B <= IA_TEX_MAX_BLOCK, "%s: block edge %d outside [%d, %d]", who, B, IA_TEX_MIN_BLOCK,
               IA_TEX_MAX_BLOCK);
  const long long want = (long long)tex_blocks_per_row(nf) * B;
  IA_CHECK_ARG(want <= IA_TEX_MAX_SIZE, "%s: %d faces in blocks of %d need an atlas of %lld texels per side, above %d", who, nf, B, want,
               IA_TEX_MAX_SIZE);
  IA_CHECK_ARG(T == (int)want, "%s: T = %d is not the atlas size %lld of %d faces in blocks of %d", who, T, want, nf, B);
  return IA_OK;
}

extern "C" int ia_tex_corner_uv(int nf, int B, int T, float *uv, void *stream) {
  if (int rc = tex_check_layout("ia_tex_corner_uv", nf, B, T)) return rc;
  if (nf == 0) return IA_OK;
  IA_CHECK_ARG(uv, "ia_tex_corner_uv: null pointer");
  hipLaunchKernelGGL(k_tex_corner_uv, dim3(ia_div_up(3ll * nf, IA_TEX_THREADS)), dim3(IA_TEX_THREADS), 0, (hipStream_t)stream, nf, B, T / B, uv);
  IA_LAUNCH_CHECK("k_tex_corner_uv");
  return IA_OK;
}

extern "C" int ia_tex_texel_points(const float *verts, int nv, const int32_t *faces, int nf, int B, int T, int first, int count,
                                   const float *t, float t_scalar, float *pts, float *normal, int32_t *owner, void *stream) {
  if (int rc = tex_check_layout("ia_tex_texel_points", nf, B, T)) return rc;
  IA_CHECK_ARG(nv >= 0, "ia_tex_texel_points: nv = %d < 0", nv);
  IA_CHECK_ARG(first >= 0 && count >= 0 && (long long)first + count <= (long long)T * T,
               "ia_tex_texel_points: texels %d .. %lld outside the atlas of %d^2", first, (long long)first + count, T);
  IA_CHECK_ARG(__builtin_isfinite(t_scalar), "ia_tex_texel_points: t_scalar is not finite");
  if (count == 0) return IA_OK;
  IA_CHECK_ARG(pts && (nf == 0 || faces) && (nf == 0 || nv == 0 || verts), "ia_tex_texel_points: null pointer");
  hipLaunchKernelGGL(k_tex_texel_points, dim3(ia_div_up(count, IA_TEX_THREADS)), dim3(IA_TEX_THREADS), 0, (hipStream_t)stream, verts, nv, faces, nf, B,
                     T, first, count, t, t_scalar, pts, normal, owner);
  IA_LAUNCH_CHECK("k_tex_texel_points");
  return IA_OK;
}

extern "C" int ia_tex_snap(const float *sigma, int K, int n, float level, float dist, const int32_t *owner, float *t_out,
                           int32_t *unsnapped, void *stream) {
  IA_CHECK_ARG(K >= IA_TEX_MIN_STEPS && K <= IA_TEX_MAX_STEPS && (K & 1), "ia_tex_snap: K = %d must be odd and in [%d, %d]", K,
               IA_TEX_MIN_STEPS, IA_TEX_MAX_STEPS);
  IA_CHECK_ARG(n >= 0, "ia_tex_snap: n = %d < 0", n);
  IA_CHECK_ARG(dist >= 0.f && __builtin_isfinite(dist), "ia_tex_snap: dist must be finite and not negative");
  IA_CHECK_ARG(__builtin_isfinite(level), "ia_tex_snap: level is not finite");
  if (n == 0) return IA_OK;
  IA_CHECK_ARG(sigma && t_out && unsnapped, "ia_tex_snap: null pointer");
  hipLaunchKernelGGL(k_tex_snap, dim3(ia_div_up(n, IA_TEX_THREADS)), dim3(IA_TEX_THREADS), 0, (hipStream_t)stream, sigma, K, n, level, dist, owner,
                     t_out, unsnapped);
  IA_LAUNCH_CHECK("k_tex_snap");
  return IA_OK;
}

extern "C" int ia_tex_sample(const float *atlas, int T, const float *uv, const float *mask, int R, float *rgb_out, void *stream) {
  IA_CHECK_ARG(T >= 1 && T <= IA_TEX_MAX_SIZE, "ia_tex_sample: T = %d outside [1, %d]", T, IA_TEX_MAX_SIZE);
  IA_CHECK_ARG(R >= 0, "ia_tex_sample: R = %d < 0", R);
  if (R == 0) return IA_OK;
  IA_CHECK_ARG(atlas && uv && rgb_out, "ia_tex_sample: null pointer");
  hipLaunchKernelGGL(k_tex_sample, dim3(ia_div_up(R, IA_TEX_THREADS)), dim3(IA_TEX_THREADS), 0, (hipStream_t)stream, atlas, T, uv, mask, R, rgb_out);
  IA_LAUNCH_CHECK("k_tex_sample");
  return IA_OK;
}
