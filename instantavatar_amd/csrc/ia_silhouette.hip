// ia_silhouette.hip -- a differentiable soft silhouette of a triangle mesh (include/instantavatar_hip_silhouette.h; definition in
// DESIGN.md section 4, "silhouette refinement"): the renderer of the `--silhouette` stage of scripts/custom/refine-smpl.py, which
// the reference takes from pytorch3d's soft rasteriser.
//
//   projection  k_sil_project_fwd / _bwd   one lane per vertex: the pinhole and its adjoint
//   set-up      k_sil_setup                one lane per face: validity, sign(A), the six screen coordinates and the face's
//                                          bounding box grown by the blur radius in pixels -> ws (both render entries run it)
//   forward     k_sil_render_fwd           one workgroup per 16 x 16 pixel tile.  It walks the faces in index order in chunks of 256:
//                                          a lane tests one box against the tile, the hits are compacted into LDS in face order
//                                          (ballot + prefix, no atomics), then every lane multiplies its pixel's prod (1 - p_f) in
//                                          that order.  A chunk never holds more than 256 hits, so the list needs no spill pass
//                                          and 8 KiB of LDS; a face that spans the image is just a hit of every tile.
//               k_sil_loss                 the tiles' partial sums of (alpha - m)^2 added in tile order
//   backward    k_sil_face_bwd             one wave per face strides over the face's grown box (a screen-filling face is 64 lanes
//                                          wide, as in k_raster_queue), recomputes p_f per pixel, and reduces its six numbers
//                                          d L / d (a, b, c) first per lane in pixel order, then over the wave in a fixed tree
//               k_sil_vertex_gather        one lane per vertex adds its corners' numbers in the order of the vertex-to-face list
// fp32 with explicit operation order (-ffp-contract=off), no atomics; every output element is written by a kernel.
#include <math.h>

#include "ia_common.h"
#include "../../include/instantavatar_hip_silhouette.h"

#define SIL_THREADS 256
#define SIL_TILE 16

struct SilTri { float ax, ay, bx, by, cx, cy, s, pad; };   // s = sign(A): +1 or -1
struct SilWs {
  float4 *box;        // [nf] grown bounding box xmin, ymin, xmax, ymax in pixels; xmin > xmax for a skipped face
  SilTri *tri;        // [nf]
  float *fgrad;       // [nf,3,2]
  float *part;        // [tiles]
  size_t bytes;
};
static SilWs sil_carve(void *ws, int nf, int H, int W) {
  WsCarver c(ws, 0);
  const size_t n = (size_t)(nf > 0 ? nf : 1);
  SilWs w;
  w.box = c.take<float4>(n);
  w.tri = c.take<SilTri>(n);
  w.fgrad = c.take<float>(n * 6);
  w.part = c.take<float>((size_t)ia_div_up(H, SIL_TILE) * ia_div_up(W, SIL_TILE));
  w.bytes = c.off;
  return w;
}
static bool sil_dims_ok(int nv, int nf, int H, int W) {
  return nv >= 0 && nf >= 0 && (long long)nf * 3 < (1LL << 31) && H >= 1 && H <= IA_SIL_MAX_DIM && W >= 1 && W <= IA_SIL_MAX_DIM;
}
extern "C" size_t ia_sil_workspace_bytes(int nv, int nf, int H, int W) {
  return sil_dims_ok(nv, nf, H, W) ? sil_carve(nullptr, nf, H, W).bytes : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// projection
// ---------------------------------------------------------------------------------------------------------------------
struct SilCam { float fx, fy, cx, cy, near; };

// p = R X + t, (u, v) and 1 / p.z of vertex i; false for an invalid vertex (every comparison is false for a NaN)
__device__ __forceinline__ bool sil_project(const float *__restrict__ verts, const float *__restrict__ w2c, const SilCam &C, int i,
                                            float *p, float *uv, float &iz) {
  const float X = verts[(size_t)i * 3], Y = verts[(size_t)i * 3 + 1], Z = verts[(size_t)i * 3 + 2];
  for (int r = 0; r < 3; r++) p[r] = ((w2c[r * 4] * X + w2c[r * 4 + 1] * Y) + w2c[r * 4 + 2] * Z) + w2c[r * 4 + 3];
  uv[0] = C.fx * p[0] / p[2] + C.cx;
  uv[1] = C.fy * p[1] / p[2] + C.cy;
  iz = 1.f / p[2];
  return p[2] >= C.near && fabsf(uv[0]) <= IA_SIL_XY_MAX && fabsf(uv[1]) <= IA_SIL_XY_MAX && iz > 0.f && iz < INFINITY;
}

__global__ __launch_bounds__(SIL_THREADS) void k_sil_project_fwd(const float *__restrict__ verts, int nv, const float *__restrict__ w2c, SilCam C,
                                                                  float *__restrict__ screen, float *__restrict__ inv_z) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nv) return;
  float p[3], uv[2], iz;
  const bool ok = sil_project(verts, w2c, C, i, p, uv, iz);
  screen[(size_t)i * 2] = ok ? uv[0] : 0.f;
  screen[(size_t)i * 2 + 1] = ok ? uv[1] : 0.f;
  inv_z[i] = ok ? iz : 0.f;
}

__global__ __launch_bounds__(SIL_THREADS) void k_sil_project_bwd(const float *__restrict__ verts, int nv, const float *__restrict__ w2c, SilCam C,
                                                                  const float *__restrict__ d_screen, float *__restrict__ d_verts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nv) return;
  float p[3], uv[2], iz, g[3] = {0.f, 0.f, 0.f};
  if (sil_project(verts, w2c, C, i, p, uv, iz)) {
    const float du = d_screen[(size_t)i * 2], dv = d_screen[(size_t)i * 2 + 1];
    const float d0 = du * C.fx / p[2], d1 = dv * C.fy / p[2];
    const float d2 = -(d0 * p[0] + d1 * p[1]) / p[2];
    for (int c = 0; c < 3; c++) g[c] = (w2c[c] * d0 + w2c[4 + c] * d1) + w2c[8 + c] * d2;
  }
  for (int c = 0; c < 3; c++) d_verts[(size_t)i * 3 + c] = g[c];
}

static int sil_camera(const char *who, float fx, float fy, float cx, float cy, float near, SilCam *C) {
  IA_CHECK_ARG(near > 0.f && near < INFINITY, "%s: near = %g is not a positive finite number", who, (double)near);
  IA_CHECK_ARG(fx == fx && fy == fy && cx == cx && cy == cy, "%s: an intrinsic is NaN", who);
  C->fx = fx; C->fy = fy; C->cx = cx; C->cy = cy; C->near = near;
  return IA_OK;
}

extern "C" int ia_sil_project_fwd(const float *verts, int nv, const float *w2c, float fx, float fy, float cx, float cy, float near,
                                  float *screen, float *inv_z, void *stream) {
  IA_CHECK_ARG(nv >= 0, "ia_sil_project_fwd: nv = %d < 0", nv);
  SilCam C;
  const int rc = sil_camera("ia_sil_project_fwd", fx, fy, cx, cy, near, &C);
  if (rc != IA_OK) return rc;
  if (nv == 0) return IA_OK;
  IA_CHECK_ARG(verts && w2c && screen && inv_z, "ia_sil_project_fwd: null pointer");
  hipLaunchKernelGGL(k_sil_project_fwd, dim3(ia_div_up(nv, SIL_THREADS)), dim3(SIL_THREADS), 0, (hipStream_t)stream, verts, nv, w2c, C, screen, inv_z);
  IA_LAUNCH_CHECK("k_sil_project_fwd");
  return IA_OK;
}

extern "C" int ia_sil_project_bwd(const float *verts, int nv, const float *w2c, float fx, float fy, float cx, float cy, float near,
                                  const float *d_screen, float *d_verts, void *stream) {
  IA_CHECK_ARG(nv >= 0, "ia_sil_project_bwd: nv = %d < 0", nv);
  SilCam C;
  const int rc = sil_camera("ia_sil_project_bwd", fx, fy, cx, cy, near, &C);
  if (rc != IA_OK) return rc;
  if (nv == 0) return IA_OK;
  IA_CHECK_ARG(verts && w2c && d_screen && d_verts, "ia_sil_project_bwd: null pointer");
  hipLaunchKernelGGL(k_sil_project_bwd, dim3(ia_div_up(nv, SIL_THREADS)), dim3(SIL_THREADS), 0, (hipStream_t)stream, verts, nv, w2c, C, d_screen, d_verts);
  IA_LAUNCH_CHECK("k_sil_project_bwd");
  return IA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// one (pixel, face) pair
// ---------------------------------------------------------------------------------------------------------------------
struct SilParams { float scale, sigma, blur, grow; int H, W; };   // scale = (2 / min(H, W))^2; grow: the blur radius in pixels, rounded up

// false when the face does not contribute to the pixel; else x_f, the winning edge k, its t and q = P - closest point
__device__ __forceinline__ bool sil_pair(const SilTri &T, float px, float py, const SilParams &P, float &x, int &kwin, float &tw, float &qx, float &qy) {
  const float vx[3] = {T.ax, T.bx, T.cx}, vy[3] = {T.ay, T.by, T.cy};
  float best = INFINITY;
  bool in = true;
  kwin = 0; tw = 0.f; qx = 0.f; qy = 0.f;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int n = (k + 1) % 3;
    const float ex = vx[n] - vx[k], ey = vy[n] - vy[k], wx = px - vx[k], wy = py - vy[k];
    float t = (wx * ex + wy * ey) / (ex * ex + ey * ey);
    t = fminf(fmaxf(t, 0.f), 1.f);
    const float rx = wx - t * ex, ry = wy - t * ey;
    const float d2 = rx * rx + ry * ry;
    in = in && T.s * (ex * wy - ey * wx) > 0.f;
    if (d2 < best) { best = d2; kwin = k; tw = t; qx = rx; qy = ry; }   // strict: the lower edge wins a tie
  }
  const float d = best * P.scale;
  if (!(in || d < P.blur)) return false;
  x = in ? d / P.sigma : -(d / P.sigma);
  return true;
}

__global__ __launch_bounds__(SIL_THREADS) void k_sil_setup(const float *__restrict__ screen, const float *__restrict__ inv_z, int nv,
                                                            const int32_t *__restrict__ faces, int nf, SilParams P, SilWs w) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
  float x[3], y[3];
  bool ok = true;
  for (int k = 0; k < 3; k++) {
    const int32_t i = faces[(size_t)f * 3 + k];
    x[k] = 0.f; y[k] = 0.f;
    if ((uint32_t)i >= (uint32_t)nv) { ok = false; continue; }
    x[k] = screen[(size_t)i * 2]; y[k] = screen[(size_t)i * 2 + 1];
    const float iz = inv_z[i];
    ok = ok && iz > 0.f && iz < INFINITY && fabsf(x[k]) <= IA_SIL_XY_MAX && fabsf(y[k]) <= IA_SIL_XY_MAX;
  }
  const float A = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0]);
  ok = ok && (A > 0.f || A < 0.f);
  SilTri T;
  T.ax = x[0]; T.ay = y[0]; T.bx = x[1]; T.by = y[1]; T.cx = x[2]; T.cy = y[2]; T.s = A > 0.f ? 1.f : -1.f; T.pad = 0.f;
  w.tri[f] = T;
  float4 b = make_float4(1.f, 1.f, 0.f, 0.f);
  if (ok) b = make_float4(fminf(x[0], fminf(x[1], x[2])) - P.grow, fminf(y[0], fminf(y[1], y[2])) - P.grow,
                          fmaxf(x[0], fmaxf(x[1], x[2])) + P.grow, fmaxf(y[0], fmaxf(y[1], y[2])) + P.grow);
  w.box[f] = b;
}

// ---------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SIL_THREADS) void k_sil_render_fwd(int nf, int tiles_x, SilParams P, SilWs w, const float *__restrict__ mask, float *__restrict__ alpha,
                                                                 float *__restrict__ d_alpha, int want_loss) {
  __shared__ SilTri s_tri[SIL_THREADS];
  __shared__ int s_wave[SIL_THREADS / IA_WAVE];
  __shared__ float s_red[SIL_THREADS];
  const int tid = threadIdx.x, lane = ia_lane(), wave = tid >> 6;
  const int tx0 = (int)(blockIdx.x % tiles_x) * SIL_TILE, ty0 = (int)(blockIdx.x / tiles_x) * SIL_TILE;
  const float fx0 = (float)tx0, fy0 = (float)ty0, fx1 = (float)(tx0 + SIL_TILE - 1), fy1 = (float)(ty0 + SIL_TILE - 1);
  const int px = tx0 + (tid & (SIL_TILE - 1)), py = ty0 + (tid >> 4);
  const float fpx = (float)px, fpy = (float)py;
  float prod = 1.f;
  for (int base = 0; base < nf; base += SIL_THREADS) {
    const int f = base + tid;
    bool hit = false;
    float4 b;
    if (f < nf) {
      b = w.box[f];
      hit = b.x <= b.z && b.x <= fx1 && b.z >= fx0 && b.y <= fy1 && b.w >= fy0;
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int pos = __popcll(m & ((1ull << lane) - 1ull)), count = 0;
    for (int q = 0; q < SIL_THREADS / IA_WAVE; q++) {
      if (q < wave) pos += s_wave[q];
      count += s_wave[q];
    }
    if (hit) s_tri[pos] = w.tri[f];
    __syncthreads();
    for (int i = 0; i < count; i++) {   // (a per-pixel test against the face's box was measured: slower, 481 -> 590 us at 540^2 -- the boxes are about a tile wide)
      float x, t, qx, qy;
      int k;
      if (sil_pair(s_tri[i], fpx, fpy, P, x, k, t, qx, qy)) prod *= 1.f / (1.f + expf(x));   // 1 - sigmoid(x), formed without the subtraction
    }
    __syncthreads();
  }
  const bool live = px < P.W && py < P.H;
  const size_t o = (size_t)py * P.W + px;
  const float a = 1.f - prod;
  float sq = 0.f;
  if (live) {
    if (alpha) alpha[o] = a;
    if (mask) {
      const float r = a - mask[o];
      sq = r * r;
      if (d_alpha) d_alpha[o] = 2.f * r / ((float)P.H * (float)P.W);
    }
  }
  if (!want_loss) return;   // (uniform)
  s_red[tid] = sq;
  __syncthreads();
  for (int s = SIL_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) s_red[tid] += s_red[tid + s];
    __syncthreads();
  }
  if (tid == 0) w.part[blockIdx.x] = s_red[0];
}

__global__ __launch_bounds__(SIL_THREADS) void k_sil_loss(const float *__restrict__ part, int n, float denom, float *__restrict__ loss) {
  __shared__ float s_red[SIL_THREADS];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += SIL_THREADS) acc += part[i];
  s_red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = SIL_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) s_red[threadIdx.x] += s_red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = s_red[0] / denom;
}

// ---------------------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SIL_THREADS) void k_sil_face_bwd(int nf, SilParams P, SilWs w, const float *__restrict__ alpha, const float *__restrict__ d_alpha) {
  const int lane = ia_lane();
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
  for (int f = wave; f < nf; f += n_waves) {   // (wave-uniform)
    const float4 b = w.box[f];
    float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // pixels at integer positions inside the grown box, clipped to the image; the comparisons are false for an empty box
    const int x0 = max((int)ceilf(b.x), 0), x1 = min((int)floorf(b.z), P.W - 1), y0 = max((int)ceilf(b.y), 0), y1 = min((int)floorf(b.w), P.H - 1);
    if (b.x <= b.z && x0 <= x1 && y0 <= y1) {
      const SilTri T = w.tri[f];
      const int bw = x1 - x0 + 1;
      const long long total = (long long)bw * (y1 - y0 + 1);
      const float c = P.scale / P.sigma;
      for (long long p = lane; p < total; p += IA_WAVE) {
        const int row = (int)(p / bw), px = x0 + (int)(p - (long long)row * bw), py = y0 + row;
        const size_t o = (size_t)py * P.W + px;
        const float up = d_alpha[o] * (1.f - alpha[o]);
        if (up == 0.f) continue;
        float x, t, qx, qy;
        int k;
        if (!sil_pair(T, (float)px, (float)py, P, x, k, t, qx, qy)) continue;
        // d L / d dist2 = up p_f (+-c): + inside (x > 0 or x == +0 on the outline), - outside
        const float pf = 1.f / (1.f + expf(-x));
        const float gd = up * pf * (signbit(x) ? -c : c);
        const float ga = -2.f * (1.f - t) * gd, gb = -2.f * t * gd;
        const int n = (k + 1) % 3;
#pragma unroll
        for (int v = 0; v < 3; v++) {
          const float s = v == k ? ga : (v == n ? gb : 0.f);
          g[v * 2] += s * qx;
          g[v * 2 + 1] += s * qy;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) g[i] += __shfl_xor(g[i], o, 64);
    if (lane < 6) {
      float v = g[0];
#pragma unroll
      for (int i = 1; i < 6; i++) v = lane == i ? g[i] : v;
      w.fgrad[(size_t)f * 6 + lane] = v;
    }
  }
}

__global__ __launch_bounds__(SIL_THREADS) void k_sil_vertex_gather(int nv, int nf, const float *__restrict__ fgrad, const int32_t *__restrict__ vf_start,
                                                                    const int32_t *__restrict__ vf_corner, float *__restrict__ d_screen) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  float gx = 0.f, gy = 0.f;
  if (nf > 0) {
    const int32_t s = vf_start[v], e = vf_start[v + 1], n = 3 * nf;
    if (s >= 0 && s <= e && e <= n)
      for (int i = s; i < e; i++) {
        const int32_t c = vf_corner[i];
        if ((uint32_t)c < (uint32_t)n) { gx += fgrad[(size_t)c * 2]; gy += fgrad[(size_t)c * 2 + 1]; }
      }
  }
  d_screen[(size_t)v * 2] = gx;
  d_screen[(size_t)v * 2 + 1] = gy;
}

static int sil_render_args(const char *who, int nv, int nf, int H, int W, float sigma, float blur, SilParams *P) {
  IA_CHECK_ARG(sil_dims_ok(nv, nf, H, W), "%s: nv = %d, nf = %d, H = %d, W = %d outside nv, nf >= 0, 3 nf < 2^31, 1 <= H, W <= %d", who, nv, nf, H, W,
               IA_SIL_MAX_DIM);
  IA_CHECK_ARG(sigma > 0.f && sigma < INFINITY, "%s: sigma = %g is not a positive finite number", who, (double)sigma);
  IA_CHECK_ARG(blur >= 0.f && blur < INFINITY, "%s: blur_radius = %g is not a finite number >= 0", who, (double)blur);
  const float c = 2.f / (float)(H < W ? H : W);
  P->scale = c * c; P->sigma = sigma; P->blur = blur; P->H = H; P->W = W;
  // the radius in pixels, rounded up generously: the box only prunes, the cut itself is the comparison d < blur_radius
  P->grow = (float)(sqrt((double)blur / (double)P->scale) * 1.001 + 0.01);
  return IA_OK;
}

extern "C" int ia_sil_render_fwd(const float *screen, const float *inv_z, int nv, const int32_t *faces, int nf, int H, int W, float sigma,
                                 float blur_radius, const float *mask, float *alpha, float *loss, float *d_alpha, void *ws, size_t ws_bytes,
                                 void *stream) {
  SilParams P;
  const int rc = sil_render_args("ia_sil_render_fwd", nv, nf, H, W, sigma, blur_radius, &P);
  if (rc != IA_OK) return rc;
  IA_CHECK_ARG(ws && (nf == 0 || (screen && inv_z && faces)), "ia_sil_render_fwd: null pointer");
  IA_CHECK_ARG(mask || (!loss && !d_alpha), "ia_sil_render_fwd: loss / d_alpha without a mask");
  const SilWs w = sil_carve(ws, nf, H, W);
  if (ws_bytes < w.bytes) return ia_set_error(IA_ERR_WORKSPACE, "ia_sil_render_fwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  if (nf > 0) {
    hipLaunchKernelGGL(k_sil_setup, dim3(ia_div_up(nf, SIL_THREADS)), dim3(SIL_THREADS), 0, s, screen, inv_z, nv, faces, nf, P, w);
    IA_LAUNCH_CHECK("k_sil_setup");
  }
  const int tiles = ia_div_up(H, SIL_TILE) * ia_div_up(W, SIL_TILE);
  hipLaunchKernelGGL(k_sil_render_fwd, dim3(tiles), dim3(SIL_THREADS), 0, s, nf, ia_div_up(W, SIL_TILE), P, w, mask, alpha, d_alpha, loss ? 1 : 0);
  IA_LAUNCH_CHECK("k_sil_render_fwd");
  if (loss) {
    hipLaunchKernelGGL(k_sil_loss, dim3(1), dim3(SIL_THREADS), 0, s, w.part, tiles, (float)H * (float)W, loss);
    IA_LAUNCH_CHECK("k_sil_loss");
  }
  return IA_OK;
}

extern "C" int ia_sil_render_bwd(const float *screen, const float *inv_z, int nv, const int32_t *faces, int nf, int H, int W, float sigma,
                                 float blur_radius, const float *alpha, const float *d_alpha, const int32_t *vf_start,
                                 const int32_t *vf_corner, float *d_screen, void *ws, size_t ws_bytes, void *stream) {
  SilParams P;
  const int rc = sil_render_args("ia_sil_render_bwd", nv, nf, H, W, sigma, blur_radius, &P);
  if (rc != IA_OK) return rc;
  IA_CHECK_ARG(ws && alpha && d_alpha && (nv == 0 || d_screen), "ia_sil_render_bwd: null pointer");
  IA_CHECK_ARG(nf == 0 || (screen && inv_z && faces && vf_start && vf_corner), "ia_sil_render_bwd: null pointer");
  const SilWs w = sil_carve(ws, nf, H, W);
  if (ws_bytes < w.bytes) return ia_set_error(IA_ERR_WORKSPACE, "ia_sil_render_bwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  if (nf > 0) {
    hipLaunchKernelGGL(k_sil_setup, dim3(ia_div_up(nf, SIL_THREADS)), dim3(SIL_THREADS), 0, s, screen, inv_z, nv, faces, nf, P, w);
    IA_LAUNCH_CHECK("k_sil_setup");
    // one wave per face, at most 8192 waves looping over the faces
    const int blocks = ia_div_up(nf, SIL_THREADS / IA_WAVE);
    hipLaunchKernelGGL(k_sil_face_bwd, dim3(blocks < 2048 ? blocks : 2048), dim3(SIL_THREADS), 0, s, nf, P, w, alpha, d_alpha);
    IA_LAUNCH_CHECK("k_sil_face_bwd");
  }
  if (nv > 0) {
    hipLaunchKernelGGL(k_sil_vertex_gather, dim3(ia_div_up(nv, SIL_THREADS)), dim3(SIL_THREADS), 0, s, nv, nf, w.fgrad, vf_start, vf_corner, d_screen);
    IA_LAUNCH_CHECK("k_sil_vertex_gather");
  }
  return IA_OK;
}
