// ia_raster.hip -- a deterministic triangle rasteriser with a z-buffer (include/instantavatar_hip_raster.h; definition in
// DESIGN.md section 4, "rasteriser"): projection to 24.8 fixed point, exact integer coverage with the top-left rule, visibility
// by a 64-bit atomic max over (inverse depth, face) keys, and a per-pixel resolve of face id, depth and interpolated attributes.
//
// Mapping.  Set-up is one lane per face.  A face whose clipped bounding box holds at most IA_RASTER_SMALL samples (a lattice-256
// mesh at 512^2: a few pixels per triangle) is rasterised by that lane; a larger one is pushed to a queue in the workspace, and
// a second kernel drains the queue with ONE WAVE per face, its lanes striding over the box, looping on the device-side count --
// a screen-filling triangle is 64 lanes wide, never one.  The queue order depends on scheduling; the image does not, because
// keys are only ever combined with max.
#include <algorithm>

#include "ia_common.h"
#include "../../include/instantavatar_hip_raster.h"

#define IA_RASTER_XY_MAX (1 << 22)
#define IA_RASTER_SMALL 16
#define IA_RASTER_THREADS 256

struct RasterHead { int32_t queued, skipped, pad[2]; };
struct RasterWs { RasterHead *head; int32_t *queue; size_t bytes; };

static RasterWs raster_carve(void *ws, int nf) {
  WsCarver c(ws, 0);
  RasterWs W;
  W.head = c.take<RasterHead>(1);
  W.queue = c.take<int32_t>((size_t)(nf > 0 ? nf : 1));
  W.bytes = c.off;
  return W;
}

static bool raster_dims_ok(int nv, int nf, int H, int W) {
  return nv >= 0 && nf >= 0 && H >= 1 && H <= IA_RASTER_MAX_DIM && W >= 1 && W <= IA_RASTER_MAX_DIM;
}

extern "C" size_t ia_raster_workspace_bytes(int nv, int nf, int H, int W) {
  if (!raster_dims_ok(nv, nf, H, W)) return 0;
  return raster_carve(nullptr, nf).bytes;
}

// ---------------------------------------------------------------------------------------------------------------------
// projection: fp64 from the fp32 inputs, rounded once (the sub-pixel position decides coverage: no fp32 cancellation in R X + t)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IA_RASTER_THREADS) void k_raster_project(const float *__restrict__ verts, int nv, const float *__restrict__ w2c,
                                                                      double fx, double fy, double cx, double cy, double near,
                                                                      int32_t *__restrict__ xy, float *__restrict__ inv_z) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nv) return;
  const double X = verts[(size_t)i * 3], Y = verts[(size_t)i * 3 + 1], Z = verts[(size_t)i * 3 + 2];
  const double px = (double)w2c[0] * X + (double)w2c[1] * Y + (double)w2c[2] * Z + (double)w2c[3];
  const double py = (double)w2c[4] * X + (double)w2c[5] * Y + (double)w2c[6] * Z + (double)w2c[7];
  const double pz = (double)w2c[8] * X + (double)w2c[9] * Y + (double)w2c[10] * Z + (double)w2c[11];
  const double u = rint((fx * px / pz + cx) * 256.0), v = rint((fy * py / pz + cy) * 256.0);
  const float w = (float)(1.0 / pz);
  // (every comparison is false for a NaN: a non-finite coordinate fails one of them)
  const bool ok = pz >= near && fabs(u) <= (double)IA_RASTER_XY_MAX && fabs(v) <= (double)IA_RASTER_XY_MAX && w > 0.f && w < INFINITY;
  xy[(size_t)i * 2] = ok ? (int32_t)u : 0;
  xy[(size_t)i * 2 + 1] = ok ? (int32_t)v : 0;
  inv_z[i] = ok ? w : 0.f;
}

extern "C" int ia_raster_project(const float *verts, int nv, const float *w2c, float fx, float fy, float cx, float cy, float near,
                                 int32_t *xy, float *inv_z, void *stream) {
  IA_CHECK_ARG(nv >= 0, "ia_raster_project: nv < 0");
  IA_CHECK_ARG(near > 0.f && near < INFINITY, "ia_raster_project: near = %g is not a positive finite number", (double)near);
  IA_CHECK_ARG(fx == fx && fy == fy && cx == cx && cy == cy, "ia_raster_project: an intrinsic is NaN");
  if (nv == 0) return IA_OK;
  IA_CHECK_ARG(verts && w2c && xy && inv_z, "ia_raster_project: null pointer");
  hipLaunchKernelGGL(k_raster_project, dim3(ia_div_up(nv, IA_RASTER_THREADS)), dim3(IA_RASTER_THREADS), 0, (hipStream_t)stream, verts, nv,
                     w2c, (double)fx, (double)fy, (double)cx, (double)cy, (double)near, xy, inv_z);
  IA_LAUNCH_CHECK("k_raster_project");
  return IA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// coverage
// ---------------------------------------------------------------------------------------------------------------------
// one face after set-up.  Edge k runs v1->v2, v2->v0, v0->v1 and starts at (ax[k], ay[k]); dx / dy carry the sign of A, so
// E_k = dx (Py - ay) - dy (Px - ax) is >= 0 inside whatever the winding; w[k] is the inverse depth of the vertex OPPOSITE edge k.
struct RasterFace {
  int32_t ax[3], ay[3], dx[3], dy[3];
  int32_t v[3];            // vertex indices: v[k] is opposite edge k
  bool tl[3];
  float w[3], area;        // area = fp32(|A|)
  int bx0, by0, bx1, by1;  // clipped bounding box in pixels, inclusive; empty when bx0 > bx1 or by0 > by1
};

enum { RASTER_SKIPPED = 0, RASTER_OK = 1 };

__device__ __forceinline__ bool raster_vertex_ok(int32_t x, int32_t y, float w) {
  return w > 0.f && w < INFINITY && x >= -IA_RASTER_XY_MAX && x <= IA_RASTER_XY_MAX && y >= -IA_RASTER_XY_MAX && y <= IA_RASTER_XY_MAX;
}

__device__ __forceinline__ int raster_setup(const int32_t *__restrict__ xy, const float *__restrict__ inv_z, int nv,
                                            const int32_t *__restrict__ faces, int f, int H, int W, int cull, RasterFace &F) {
  int32_t x[3], y[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int32_t i = faces[(size_t)f * 3 + k];
    if ((uint32_t)i >= (uint32_t)nv) return RASTER_SKIPPED;
    F.v[k] = i;
    x[k] = xy[(size_t)i * 2]; y[k] = xy[(size_t)i * 2 + 1]; F.w[k] = inv_z[i];
    if (!raster_vertex_ok(x[k], y[k], F.w[k])) return RASTER_SKIPPED;
  }
  const long long A = (long long)(x[1] - x[0]) * (y[2] - y[0]) - (long long)(x[2] - x[0]) * (y[1] - y[0]);
  if (A == 0 || (cull && A > 0)) return RASTER_SKIPPED;
  const int s = A > 0 ? 1 : -1;
  F.area = (float)(A > 0 ? A : -A);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    F.ax[k] = x[a]; F.ay[k] = y[a];
    F.dx[k] = s * (x[b] - x[a]); F.dy[k] = s * (y[b] - y[a]);
    F.tl[k] = F.dy[k] < 0 || (F.dy[k] == 0 && F.dx[k] > 0);
  }
  const int xmin = min(x[0], min(x[1], x[2])), xmax = max(x[0], max(x[1], x[2]));
  const int ymin = min(y[0], min(y[1], y[2])), ymax = max(y[0], max(y[1], y[2]));
  // samples sit at multiples of 256: the first at or after the minimum, the last at or before the maximum (>> floors)
  F.bx0 = max((xmin + 255) >> 8, 0); F.bx1 = min(xmax >> 8, W - 1);
  F.by0 = max((ymin + 255) >> 8, 0); F.by1 = min(ymax >> 8, H - 1);
  return RASTER_OK;
}

// the three edge functions at the sample of pixel (px, py); true when it is covered
__device__ __forceinline__ bool raster_edges(const RasterFace &F, int px, int py, long long e[3]) {
  const int Px = px << 8, Py = py << 8;
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    e[k] = (long long)F.dx[k] * (Py - F.ay[k]) - (long long)F.dy[k] * (Px - F.ax[k]);
    in = in && (e[k] > 0 || (e[k] == 0 && F.tl[k]));
  }
  return in;
}

__device__ __forceinline__ void raster_fragment(const RasterFace &F, int f, int px, int py, int W, unsigned long long *__restrict__ vis) {
  long long e[3];
  if (!raster_edges(F, px, py, e)) return;
  const float l0 = (float)e[0] / F.area, l1 = (float)e[1] / F.area, l2 = (float)e[2] / F.area;
  const float iz = IA_DOT3(l0, F.w[0], l1, F.w[1], l2, F.w[2]);
  const unsigned long long key = ((unsigned long long)__float_as_uint(iz) << 32) | (0xFFFFFFFFu - (uint32_t)f);
  unsigned long long *cell = vis + (size_t)py * W + px;
  // keys only grow: a stale pre-read can only let a superfluous atomic through, never drop a winner
  if (__hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(cell, key);
}

__global__ __launch_bounds__(IA_RASTER_THREADS) void k_raster_clear(unsigned long long *__restrict__ vis, size_t n, RasterHead *head) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) vis[i] = 0ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) { head->queued = 0; head->skipped = 0; head->pad[0] = 0; head->pad[1] = 0; }
}

__global__ __launch_bounds__(IA_RASTER_THREADS) void k_raster_faces(const int32_t *__restrict__ xy, const float *__restrict__ inv_z, int nv,
                                                                    const int32_t *__restrict__ faces, int nf, int H, int W, int cull,
                                                                    unsigned long long *__restrict__ vis, RasterHead *head,
                                                                    int32_t *__restrict__ queue) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  RasterFace F;
  const bool live = f < nf;
  const bool skipped = live && raster_setup(xy, inv_z, nv, faces, f, H, W, cull, F) == RASTER_SKIPPED;
  // one add per wave: the count of its skipped faces
  const unsigned long long sk = __ballot(skipped);
  if (sk && ia_lane() == __ffsll((long long)sk) - 1) atomicAdd(&head->skipped, __popcll(sk));
  if (!live || skipped || F.bx0 > F.bx1 || F.by0 > F.by1) return;
  const int bw = F.bx1 - F.bx0 + 1, bh = F.by1 - F.by0 + 1;
  if ((long long)bw * bh > IA_RASTER_SMALL) {
    queue[atomicAdd(&head->queued, 1)] = f;      // at most one entry per face: the queue holds nf
    return;
  }
  for (int py = F.by0; py <= F.by1; py++)
    for (int px = F.bx0; px <= F.bx1; px++) raster_fragment(F, f, px, py, W, vis);
}

__global__ __launch_bounds__(IA_RASTER_THREADS) void k_raster_queue(const int32_t *__restrict__ xy, const float *__restrict__ inv_z, int nv,
                                                                    const int32_t *__restrict__ faces, int nf, int H, int W, int cull,
                                                                    unsigned long long *__restrict__ vis, const RasterHead *__restrict__ head,
                                                                    const int32_t *__restrict__ queue) {
  const int lane = ia_lane();
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
  const int n = min(head->queued, nf);
  for (int q = wave; q < n; q += n_waves) {
    const int f = queue[q];
    RasterFace F;
    if ((uint32_t)f >= (uint32_t)nf || raster_setup(xy, inv_z, nv, faces, f, H, W, cull, F) != RASTER_OK) continue;   // (wave-uniform)
    const int bw = F.bx1 - F.bx0 + 1, bh = F.by1 - F.by0 + 1;
    const int total = bw * bh;       // <= 2^28
    for (int p = lane; p < total; p += IA_WAVE) {
      const int row = p / bw;
      raster_fragment(F, f, F.bx0 + (p - row * bw), F.by0 + row, W, vis);
    }
  }
}

extern "C" int ia_raster_visibility(const int32_t *xy, const float *inv_z, int nv, const int32_t *faces, int nf, int H, int W, int cull,
                                    int64_t *vis, void *ws, size_t ws_bytes, void *stream) {
  IA_CHECK_ARG(raster_dims_ok(nv, nf, H, W), "ia_raster_visibility: nv = %d, nf = %d, H = %d, W = %d outside nv, nf >= 0, 1 <= H, W <= %d",
               nv, nf, H, W, IA_RASTER_MAX_DIM);
  IA_CHECK_ARG(vis && ws && (nf == 0 || (xy && inv_z && faces)), "ia_raster_visibility: null pointer");
  const RasterWs R = raster_carve(ws, nf);
  if (ws_bytes < R.bytes) return ia_set_error(IA_ERR_WORKSPACE, "ia_raster_visibility: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)H * W;
  unsigned long long *v = (unsigned long long *)vis;
  hipLaunchKernelGGL(k_raster_clear, dim3((int)std::min<size_t>((n + IA_RASTER_THREADS - 1) / IA_RASTER_THREADS, 2048)), dim3(IA_RASTER_THREADS),
                     0, s, v, n, R.head);
  if (nf > 0) {
    hipLaunchKernelGGL(k_raster_faces, dim3(ia_div_up(nf, IA_RASTER_THREADS)), dim3(IA_RASTER_THREADS), 0, s, xy, inv_z, nv, faces, nf, H, W,
                       cull, v, R.head, R.queue);
    // one wave per queued face, at most 8192 waves looping on the device-side count
    hipLaunchKernelGGL(k_raster_queue, dim3(std::min(ia_div_up(nf, IA_RASTER_THREADS / IA_WAVE), 2048)), dim3(IA_RASTER_THREADS), 0, s, xy,
                       inv_z, nv, faces, nf, H, W, cull, v, R.head, R.queue);
  }
  IA_LAUNCH_CHECK("k_raster_queue");
  return IA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// resolve: one lane per pixel
// ---------------------------------------------------------------------------------------------------------------------
__global__ void k_raster_counts(const RasterHead *__restrict__ head, int32_t *__restrict__ counts) {
  counts[0] = head->skipped;
  counts[1] = 0;
}

__global__ __launch_bounds__(IA_RASTER_THREADS) void k_raster_resolve(const int32_t *__restrict__ xy, const float *__restrict__ inv_z, int nv,
                                                                      const int32_t *__restrict__ faces, int nf,
                                                                      const unsigned long long *__restrict__ vis, int H, int W,
                                                                      const float *__restrict__ attrs, int C, int32_t *__restrict__ face_id,
                                                                      float *__restrict__ depth, float *__restrict__ attr_out,
                                                                      int32_t *__restrict__ counts) {
  const size_t n = (size_t)H * W;
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long key = p < n ? vis[p] : 0ull;
  const uint32_t f = 0xFFFFFFFFu - (uint32_t)key;
  const bool hit = key != 0ull && f < (uint32_t)nf;
  const unsigned long long hits = __ballot(hit);
  if (hits && ia_lane() == __ffsll((long long)hits) - 1) atomicAdd(&counts[1], __popcll(hits));
  if (p >= n) return;
  const float iz = __uint_as_float((uint32_t)(key >> 32));
  face_id[p] = hit ? (int32_t)f : -1;
  depth[p] = hit ? 1.f / iz : 0.f;
  if (C <= 0) return;
  float out[IA_RASTER_MAX_CHANNELS];
#pragma unroll
  for (int c = 0; c < IA_RASTER_MAX_CHANNELS; c++) out[c] = 0.f;
  RasterFace F;
  if (hit && raster_setup(xy, inv_z, nv, faces, (int)f, H, W, 0, F) == RASTER_OK) {
    long long e[3];
    const uint32_t row = (uint32_t)p / (uint32_t)W;      // p < 2^28
    raster_edges(F, (int)((uint32_t)p - row * (uint32_t)W), (int)row, e);
    const float t0 = (float)e[0] / F.area * F.w[0], t1 = (float)e[1] / F.area * F.w[1], t2 = (float)e[2] / F.area * F.w[2];
    const float *a0 = attrs + (size_t)F.v[0] * C, *a1 = attrs + (size_t)F.v[1] * C, *a2 = attrs + (size_t)F.v[2] * C;
#pragma unroll
    for (int c = 0; c < IA_RASTER_MAX_CHANNELS; c++)
      if (c < C) out[c] = IA_DOT3(t0, a0[c], t1, a1[c], t2, a2[c]) / iz;
  }
#pragma unroll
  for (int c = 0; c < IA_RASTER_MAX_CHANNELS; c++)
    if (c < C) attr_out[p * C + c] = out[c];
}

extern "C" int ia_raster_resolve(const int32_t *xy, const float *inv_z, int nv, const int32_t *faces, int nf, const int64_t *vis, int H,
                                 int W, const float *attrs, int C, const void *ws, size_t ws_bytes, int32_t *face_id, float *depth,
                                 float *attr_out, int32_t *counts, void *stream) {
  IA_CHECK_ARG(raster_dims_ok(nv, nf, H, W), "ia_raster_resolve: nv = %d, nf = %d, H = %d, W = %d outside nv, nf >= 0, 1 <= H, W <= %d",
               nv, nf, H, W, IA_RASTER_MAX_DIM);
  IA_CHECK_ARG(C >= 0 && C <= IA_RASTER_MAX_CHANNELS, "ia_raster_resolve: C = %d outside [0, %d]", C, IA_RASTER_MAX_CHANNELS);
  IA_CHECK_ARG(vis && ws && face_id && depth && counts, "ia_raster_resolve: null pointer");
  IA_CHECK_ARG(C == 0 || (attrs && attr_out), "ia_raster_resolve: C = %d without attrs / attr_out", C);
  IA_CHECK_ARG(nf == 0 || (xy && inv_z && faces), "ia_raster_resolve: null pointer");
  const RasterWs R = raster_carve(const_cast<void *>(ws), nf);
  if (ws_bytes < R.bytes) return ia_set_error(IA_ERR_WORKSPACE, "ia_raster_resolve: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)H * W;
  hipLaunchKernelGGL(k_raster_counts, dim3(1), dim3(1), 0, s, R.head, counts);
  hipLaunchKernelGGL(k_raster_resolve, dim3((unsigned)((n + IA_RASTER_THREADS - 1) / IA_RASTER_THREADS)), dim3(IA_RASTER_THREADS), 0, s, xy,
                     inv_z, nv, faces, nf, (const unsigned long long *)vis, H, W, attrs, C, face_id, depth, attr_out, counts);
  IA_LAUNCH_CHECK("k_raster_resolve");
  return IA_OK;
}
