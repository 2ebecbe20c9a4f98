// ia_phototex.hip -- a photo texture (no counterpart in the reference): the frames a sequence was recorded with, projected back onto
// the texture atlas of the mesh (layout of ia_mesh_dev.h, the one ia_texture.hip bakes through; camera of ia_raster.hip).
//   zero-fill of the fp64 accumulator                                       (ia_phototex_zero)
//   a chunk of frames added to a range of texels                            (ia_phototex_accumulate)
//   the weighted mean, the fallback atlas and the per-texel frame count     (ia_phototex_resolve)
// The definition is stated in DESIGN.md section 4 ("photo texture") and in include/instantavatar_hip_phototex.h.  Every decision and
// sum is fp64 on the fp32 inputs, the frames of a texel are added in ascending order starting from what its record holds, and no
// two threads share a record: two calls give the same bytes, however frames and texels are split.  Nothing here synchronises,
// allocates or reads on the host; the only atomic adds integers.
//
// k_phototex_accumulate: one workgroup per block of the atlas (two faces, B^2 texels; B = 8 is one wave), so the owner face and its
// posed corners take two values per wave and the camera rows are uniform.  A lane keeps S, W and seen of its texel in registers over
// the frames of the call and touches its record once.
#include "ia_common.h"
#include "ia_mesh_dev.h"
#include "../../include/instantavatar_hip_phototex.h"
#include "../../include/instantavatar_hip_texture.h"

#define IA_PHOTOTEX_THREADS 256

namespace {

struct PhotoRecord {          // IA_PHOTOTEX_ACC_STRIDE bytes
  double s0, s1, s2, w;
  int32_t seen, unused;
};
static_assert(sizeof(PhotoRecord) == IA_PHOTOTEX_ACC_STRIDE, "the accumulator record is IA_PHOTOTEX_ACC_STRIDE bytes");

struct PhotoCamera {
  double fx, fy, cx, cy, near;
};

__global__ __launch_bounds__(IA_PHOTOTEX_THREADS) void k_phototex_zero(unsigned long long *__restrict__ acc, long long words) {
  const long long i = (long long)blockIdx.x * IA_PHOTOTEX_THREADS + threadIdx.x;
  if (i < words) acc[i] = 0ull;
}

// the contribution of frame `fr` to one texel with weights bw on the face with corners idx; false: nothing
__device__ __forceinline__ bool ptx_frame(const float *__restrict__ verts, int nv, const int idx[3], const double bw[3], int fr, const float *__restrict__ w2c, const PhotoCamera &cam,
                                          const uint8_t *__restrict__ images, const float *__restrict__ masks,
                                          const float *__restrict__ depth, int H, int W, double cos_min, double power, double depth_tol,
                                          double &r0, double &r1, double &r2, double &wgt) {
  double c3[3][3], pt[3], m[3];
  ia_face_corners(verts + (size_t)fr * nv * 3, idx, c3);
  if (!ia_corners_finite(c3)) return false;
  ia_face_point(c3, bw, pt);
  const double p0 = pt[0], p1 = pt[1], p2 = pt[2];
  const float *M = w2c + 16 * (size_t)fr;
  const double R00 = M[0], R01 = M[1], R02 = M[2], R10 = M[4], R11 = M[5], R12 = M[6], R20 = M[8], R21 = M[9], R22 = M[10];
  const double x0 = R00 * p0 + R01 * p1 + R02 * p2 + (double)M[3];
  const double x1 = R10 * p0 + R11 * p1 + R12 * p2 + (double)M[7];
  const double x2 = R20 * p0 + R21 * p1 + R22 * p2 + (double)M[11];
  if (!(x2 >= cam.near)) return false;
  const double u = cam.fx * x0 / x2 + cam.cx, vv = cam.fy * x1 / x2 + cam.cy;
  if (!(u >= 0.0 && u < (double)(W - 1) && vv >= 0.0 && vv < (double)(H - 1))) return false;      // NaN fails
  // facing
  ia_face_cross(c3, m);
  const double len = ia_len3d(m);
  if (!(len > 0.0 && __builtin_isfinite(len))) return false;
  const double n0 = m[0] / len, n1 = m[1] / len, n2 = m[2] / len;
  const double q0 = R00 * n0 + R01 * n1 + R02 * n2, q1 = R10 * n0 + R11 * n1 + R12 * n2, q2 = R20 * n0 + R21 * n1 + R22 * n2;
  const double c = -(q0 * x0 + q1 * x1 + q2 * x2) / sqrt(x0 * x0 + x1 * x1 + x2 * x2);
  if (!(c > cos_min)) return false;
  // footprint: i0 in [0, W - 2], j0 in [0, H - 2]
  const double uf = floor(u), vf = floor(vv);
  const int i0 = (int)uf, j0 = (int)vf;
  const size_t px = ((size_t)fr * H + j0) * W + i0;          // pixel (i0, j0) of the frame; (i0 + 1, j0 + 1) is px + W + 1, inside
  const size_t at[4] = {px, px + 1, px + W, px + (size_t)W + 1};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (masks && !(masks[at[k]] >= 0.5f)) return false;
    const double d = depth[at[k]];
    if (!(d > 0.0) || !(fabs(x2 - d) <= depth_tol)) return false;
  }
  const double fu = u - uf, fv = vv - vf;
  double rgb[3];
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    const double c00 = images[3 * at[0] + ch], c10 = images[3 * at[1] + ch], c01 = images[3 * at[2] + ch], c11 = images[3 * at[3] + ch];
    const double top = c00 + fu * (c10 - c00), bot = c01 + fu * (c11 - c01);
    rgb[ch] = (top + fv * (bot - top)) / 255.0;
  }
  wgt = power == 2.0 ? c * c : (power == 0.0 ? 1.0 : (power == 1.0 ? c : pow(c, power)));
  r0 = rgb[0];
  r1 = rgb[1];
  r2 = rgb[2];
  return true;
}

// grid: (blocks per atlas row, block rows that the texel range touches); br0: the first of those block rows
__global__ __launch_bounds__(IA_PHOTOTEX_THREADS) void k_phototex_accumulate(
    const float *__restrict__ verts, int nv, const int32_t *__restrict__ faces, int nf, int B, int T, int first, int count, int F,
    const float *__restrict__ w2c, PhotoCamera cam, const uint8_t *__restrict__ images, const float *__restrict__ masks,
    const float *__restrict__ depth, int H, int W, double cos_min, double power, double depth_tol, PhotoRecord *__restrict__ acc, int br0) {
  const int bc = blockIdx.x, br = br0 + blockIdx.y;
  const int nb = T / B;
  for (int k = threadIdx.x; k < B * B; k += blockDim.x) {
    int j = k / B, i = k - j * B;
    const long long g = (long long)(br * B + j) * T + (bc * B + i);           // < T^2 <= 2^28
    if (g < first || g >= (long long)first + count) continue;
    const int h = ia_atlas_half(B, i, j);
    const int f = ia_atlas_face(br, bc, nb, h);
    if (f >= nf) continue;
    int idx[3];
    ia_face_load(faces, f, idx);
    if (!ia_face_in_range(idx, nv)) continue;
    double u[3];
    ia_atlas_weights(B, i, j, u);
    PhotoRecord *rec = acc + (size_t)(g - first);
    double s0 = rec->s0, s1 = rec->s1, s2 = rec->s2, w = rec->w;
    int seen = rec->seen;
    for (int fr = 0; fr < F; fr++) {
      double r0, r1, r2, wgt;
      if (ptx_frame(verts, nv, idx, u, fr, w2c, cam, images, masks, depth, H, W, cos_min, power, depth_tol, r0, r1, r2, wgt)) {
        s0 += wgt * r0;
        s1 += wgt * r1;
        s2 += wgt * r2;
        w += wgt;
        seen++;
      }
    }
    rec->s0 = s0;
    rec->s1 = s1;
    rec->s2 = s2;
    rec->w = w;
    rec->seen = seen;
  }
}

__global__ __launch_bounds__(IA_PHOTOTEX_THREADS) void k_phototex_resolve(const PhotoRecord *__restrict__ acc, const float *__restrict__ base,
                                                                          const int32_t *__restrict__ owner, int count, int min_frames,
                                                                          float *__restrict__ atlas, int32_t *__restrict__ seen_out,
                                                                          int32_t *__restrict__ unseen) {
  const int i = blockIdx.x * IA_PHOTOTEX_THREADS + threadIdx.x;
  bool miss = false;
  if (i < count) {
    const PhotoRecord r = acc[i];
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    if (owner[i] >= 0) {
      if (r.seen >= min_frames) {
        c0 = (float)(r.s0 / r.w);
        c1 = (float)(r.s1 / r.w);
        c2 = (float)(r.s2 / r.w);
      } else if (base) {
        c0 = base[3 * (size_t)i];
        c1 = base[3 * (size_t)i + 1];
        c2 = base[3 * (size_t)i + 2];
      }
      miss = r.seen == 0;
    }
    atlas[3 * (size_t)i] = c0;
    atlas[3 * (size_t)i + 1] = c1;
    atlas[3 * (size_t)i + 2] = c2;
    seen_out[i] = r.seen;
  }
  // one integer atomic per wave
  const unsigned long long b = __ballot(miss);
  if (ia_lane() == 0 && b) atomicAdd(unseen, __popcll(b));
}

}  // namespace

extern "C" size_t ia_phototex_acc_bytes(int count) { return count < 0 ? 0 : (size_t)count * IA_PHOTOTEX_ACC_STRIDE; }

extern "C" int ia_phototex_zero(void *acc, int count, void *stream) {
  IA_CHECK_ARG(count >= 0, "ia_phototex_zero: count = %d < 0", count);
  if (count == 0) return IA_OK;
  IA_CHECK_ARG(acc, "ia_phototex_zero: null pointer");
  IA_CHECK_ARG(((uintptr_t)acc & 7) == 0, "ia_phototex_zero: the accumulator is not 8-byte aligned");
  const long long words = (long long)count * (IA_PHOTOTEX_ACC_STRIDE / 8);
  hipLaunchKernelGGL(k_phototex_zero, dim3(ia_div_up(words, IA_PHOTOTEX_THREADS)), dim3(IA_PHOTOTEX_THREADS), 0, (hipStream_t)stream,
                     (unsigned long long *)acc, words);
  IA_LAUNCH_CHECK("k_phototex_zero");
  return IA_OK;
}

extern "C" int ia_phototex_accumulate(const float *verts, int nv, const int32_t *faces, int nf, int B, int T, int first, int count, int F,
                                      const float *w2c, float fx, float fy, float cx, float cy, float near, const uint8_t *images,
                                      const float *masks, const float *depth, int H, int W, float cos_min, float power, float depth_tol,
                                      void *acc, void *stream) {
  const char *who = "ia_phototex_accumulate";
  IA_CHECK_ARG(nf >= 0, "%s: nf = %d < 0", who, nf);
  IA_CHECK_ARG(nv >= 0, "%s: nv = %d < 0", who, nv);
  IA_CHECK_ARG(B >= IA_TEX_MIN_BLOCK && B <= IA_TEX_MAX_BLOCK, "%s: block edge %d outside [%d, %d]", who, B, IA_TEX_MIN_BLOCK,
               IA_TEX_MAX_BLOCK);
  const int want = ia_tex_atlas_size(nf, B);
  IA_CHECK_ARG(want > 0, "%s: %d faces in blocks of %d need an atlas above %d texels per side", who, nf, B, IA_TEX_MAX_SIZE);
  IA_CHECK_ARG(T == want, "%s: T = %d is not the atlas size %d of %d faces in blocks of %d", who, T, want, nf, B);
  IA_CHECK_ARG(first >= 0 && count >= 0 && (long long)first + count <= (long long)T * T, "%s: texels %d .. %lld outside the atlas of %d^2",
               who, first, (long long)first + count, T);
  IA_CHECK_ARG(F >= 1 && F <= IA_PHOTOTEX_MAX_FRAMES, "%s: F = %d outside [1, %d]", who, F, IA_PHOTOTEX_MAX_FRAMES);
  IA_CHECK_ARG(H >= 1 && H <= IA_PHOTOTEX_MAX_DIM && W >= 1 && W <= IA_PHOTOTEX_MAX_DIM, "%s: a %d x %d image: outside 1 <= H, W <= %d", who,
               H, W, IA_PHOTOTEX_MAX_DIM);
  IA_CHECK_ARG(__builtin_isfinite(fx) && __builtin_isfinite(fy) && __builtin_isfinite(cx) && __builtin_isfinite(cy),
               "%s: the intrinsics are not finite", who);
  IA_CHECK_ARG(near > 0.f && __builtin_isfinite(near), "%s: near must be positive and finite", who);
  IA_CHECK_ARG(cos_min >= 0.f && cos_min < 1.f, "%s: cos_min = %g outside [0, 1)", who, (double)cos_min);
  IA_CHECK_ARG(power >= 0.f && __builtin_isfinite(power), "%s: power = %g must be finite and not negative", who, (double)power);
  IA_CHECK_ARG(depth_tol >= 0.f && __builtin_isfinite(depth_tol), "%s: depth_tol = %g must be finite and not negative", who,
               (double)depth_tol);
  if (count == 0 || nf == 0) return IA_OK;
  IA_CHECK_ARG(faces && (nv == 0 || verts) && w2c && images && depth && acc, "%s: null pointer", who);
  IA_CHECK_ARG(((uintptr_t)acc & 7) == 0, "%s: the accumulator is not 8-byte aligned", who);
  const int br0 = (first / T) / B, br1 = (int)((((long long)first + count - 1) / T) / B);
  const int threads = B * B >= IA_PHOTOTEX_THREADS ? IA_PHOTOTEX_THREADS : (B * B + IA_WAVE - 1) / IA_WAVE * IA_WAVE;
  PhotoCamera cam = {(double)fx, (double)fy, (double)cx, (double)cy, (double)near};
  hipLaunchKernelGGL(k_phototex_accumulate, dim3(T / B, br1 - br0 + 1), dim3(threads), 0, (hipStream_t)stream, verts, nv, faces, nf, B, T,
                     first, count, F, w2c, cam, images, masks, depth, H, W, (double)cos_min, (double)power, (double)depth_tol,
                     (PhotoRecord *)acc, br0);
  IA_LAUNCH_CHECK("k_phototex_accumulate");
  return IA_OK;
}

extern "C" int ia_phototex_resolve(const void *acc, const float *base, const int32_t *owner, int count, int min_frames, float *atlas,
                                   int32_t *seen, int32_t *unseen, void *stream) {
  IA_CHECK_ARG(count >= 0, "ia_phototex_resolve: count = %d < 0", count);
  IA_CHECK_ARG(min_frames >= 1, "ia_phototex_resolve: min_frames = %d < 1", min_frames);
  if (count == 0) return IA_OK;
  IA_CHECK_ARG(acc && owner && atlas && seen && unseen, "ia_phototex_resolve: null pointer");
  IA_CHECK_ARG(((uintptr_t)acc & 7) == 0, "ia_phototex_resolve: the accumulator is not 8-byte aligned");
  hipLaunchKernelGGL(k_phototex_resolve, dim3(ia_div_up(count, IA_PHOTOTEX_THREADS)), dim3(IA_PHOTOTEX_THREADS), 0, (hipStream_t)stream,
                     (const PhotoRecord *)acc, base, owner, count, min_frames, atlas, seen, unseen);
  IA_LAUNCH_CHECK("k_phototex_resolve");
  return IA_OK;
}
