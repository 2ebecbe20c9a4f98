// ia_keypoints.hip -- the loss of the custom pipeline's SMPL refinement over all frames of a sequence, and its gradient (gfx950).
//
// Reference: scripts/custom/refine-smpl.py:187-208 -- smplx's SMPL.forward on F frames at once, the BODY_25 joint mapper
// (:74-84), a pinhole projection (:30-33), the masked Euclidean keypoint error and a temporal term on the posed vertices, under
// autograd and Adam.  Definition: DESIGN.md section 4, "keypoint refinement"; C ABI: include/instantavatar_hip_keypoints.h.
//
//   forward   k_kp_check        validates the device copy of kp_vertex (the host waits for its flag before anything else runs)
//             k_kp_chain_fwd    one wave per frame: J = J0 + JS beta, Rodrigues, the chain -> A (no translation), pose feature, joints
//             k_kp_vertex_fwd   one thread per vertex and KP_FT frames per block: the tile's pose features and A matrices sit in
//                               LDS, so one pass over posedirs serves the whole tile -> verts
//             k_kp_points       the 35 model points, their projections, the per-keypoint error
//             k_kp_temporal     |vert[f+1,v] - vert[f,v]| summed into per-block partials;  k_kp_loss_final: the three loss terms
//   backward  k_kp_chain_fwd, then
//             k_kp_point_grad   d loss / d model point [F,35,3] (keypoint term)
//             k_kp_vertex_bwd   d vert[f,v] formed analytically from verts[f-1], verts[f], verts[f+1] and the sparse keypoint
//                               shares (no [F,V,3] gradient buffer), staged in LDS per tile and summed over the block's vertices
//                               in vertex order into per-block partials of d A (288), d pf (207), d betas (10), d transl (3)
//             k_kp_reduce_v     partials summed over the vertex blocks in block order
//             k_kp_chain_bwd    one wave per frame: the chain reversed, Rodrigues backward -> d pose, d transl, the frame's d betas
//             k_kp_reduce_f     d betas summed over the frames in frame order
//   adjoint   ia_sil_body_bwd (include/instantavatar_hip_silhouette.h): the same backward for a vertex cotangent handed in by the
//             caller -- k_kp_vertex_bwd<true> reads d vert[f,v] instead of forming it, d point is zero-filled, the rest is shared
// fp32 with explicit operation order (-ffp-contract=off), every sum in a fixed order, no atomics.
#include "ia_common.h"
#include "ia_smpl_dev.h"
#include "../../include/instantavatar_hip_keypoints.h"
#include "../../include/instantavatar_hip_silhouette.h"

#define KP_THREADS 256
#define KP_FT 4             // frames per tile of the vertex kernels
#define KP_PF 208           // row stride of the pose features (207 used)
#define KP_NOUT 508         // per frame: d A [24,12], d pf [207], d betas through the shape blend [10], d transl [3]
#define KP_O_PF 288
#define KP_O_BETA 495
#define KP_O_TR 505
#define KP_TBLOCKS 512      // at most this many partial sums of the temporal term

// BODY_25 point k is model point KP_MAP[k] (refine-smpl.py:75-78); MidHip (k = 8) is not in the loss (:133-134)
__constant__ int KP_MAP[IA_KP_N_BODY25] = {24, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34};
#define KP_MIDHIP 8

struct KpBodyDev {
  const float *v_template, *shapedirs, *posedirs, *lbs_weights, *J0, *JS;
  const int32_t *parents;
  int V;
};

struct KpWs {
  int32_t *flag;                               // [64]
  float *A, *pf, *joints;                      // [F,288] [F,KP_PF] [F,72]
  float *verts, *points, *uv, *e, *tpart;      // [F,V,3] [F,35,3] [F,25,2] [F,25] [KP_TBLOCKS]
  float *dpoint, *part, *red, *dbf;            // [F,35,3] [F,VB,KP_NOUT] [F,KP_NOUT] [F,10]
  size_t bytes;
};
static KpWs kp_carve(void *ws, int F, int V) {
  WsCarver c(ws, 0);
  const size_t f = (size_t)F, vb = (size_t)ia_div_up(V, KP_THREADS);
  KpWs w;
  w.flag = c.take<int32_t>(64);
  w.A = c.take<float>(f * 288); w.pf = c.take<float>(f * KP_PF); w.joints = c.take<float>(f * 72);
  w.verts = c.take<float>(f * V * 3); w.points = c.take<float>(f * IA_KP_N_POINTS * 3); w.uv = c.take<float>(f * IA_KP_N_BODY25 * 2);
  w.e = c.take<float>(f * IA_KP_N_BODY25); w.tpart = c.take<float>(KP_TBLOCKS);
  w.dpoint = c.take<float>(f * IA_KP_N_POINTS * 3); w.part = c.take<float>(f * vb * KP_NOUT); w.red = c.take<float>(f * KP_NOUT);
  w.dbf = c.take<float>(f * 10);
  w.bytes = c.off;
  return w;
}
static inline bool kp_sizes_ok(int F, int V) { return F >= 1 && V >= 1 && (long long)F * V * 3 < (1LL << 31); }
extern "C" size_t ia_kp_workspace_bytes(int n_frames, int n_verts) {
  return kp_sizes_ok(n_frames, n_verts) ? kp_carve(nullptr, n_frames, n_verts).bytes : 0;
}

__global__ void k_kp_check(const int32_t *__restrict__ kp_vertex, int V, int32_t *__restrict__ flag) {
  if (threadIdx.x == 0) {
    int bad = 0;
    for (int m = 0; m < IA_KP_N_VERTEX; m++) bad |= (kp_vertex[m] < 0 || kp_vertex[m] >= V) ? 1 : 0;
    flag[0] = bad;
  }
}

__global__ void k_kp_chain_fwd(KpBodyDev B, const float *__restrict__ betas, const float *__restrict__ pose, KpWs w) {
  __shared__ float R[24][9], Jn[24][3], G[24][12];
  __shared__ int par[24];
  const int j = threadIdx.x;
  const size_t f = blockIdx.x;
  if (j < 24) {
    par[j] = B.parents[j];
    for (int c = 0; c < 3; c++) {   // J = J0 + JS beta (lbs.py:185-190, regressor folded)
      float v = B.J0[j * 3 + c];
      for (int l = 0; l < 10; l++) v += B.JS[(j * 3 + c) * 10 + l] * betas[l];
      Jn[j][c] = v;
    }
    Rod r;
    rodrigues(pose + f * 72 + j * 3, r);
    for (int a = 0; a < 9; a++) R[j][a] = r.R[a];
    if (j >= 1)
      for (int a = 0; a < 9; a++) w.pf[f * KP_PF + (j - 1) * 9 + a] = r.R[a] - ((a == 0 || a == 4 || a == 8) ? 1.f : 0.f);
  }
  __syncthreads();
  chain_forward(R, Jn, par, G, j);
  if (j < 24)
    for (int a = 0; a < 3; a++) {
      const float t = G[j][a * 4] * Jn[j][0] + G[j][a * 4 + 1] * Jn[j][1] + G[j][a * 4 + 2] * Jn[j][2];
      for (int b = 0; b < 3; b++) w.A[f * 288 + j * 12 + a * 4 + b] = G[j][a * 4 + b];
      w.A[f * 288 + j * 12 + a * 4 + 3] = G[j][a * 4 + 3] - t;
      w.joints[f * 72 + j * 3 + a] = G[j][a * 4 + 3];
    }
}

// the tile's A and pose features into LDS; rows of frames past the last are zero
__device__ __forceinline__ void kp_load_tile(const KpWs &w, int f0, int F, float (*sA)[288], float (*spf)[KP_PF]) {
  for (int i = threadIdx.x; i < KP_FT * 288; i += KP_THREADS) sA[i / 288][i % 288] = f0 + i / 288 < F ? w.A[(size_t)f0 * 288 + i] : 0.f;
  for (int i = threadIdx.x; i < KP_FT * KP_PF; i += KP_THREADS)
    spf[i / KP_PF][i % KP_PF] = (f0 + i / KP_PF < F && i % KP_PF < 207) ? w.pf[(size_t)f0 * KP_PF + i] : 0.f;
}

// pose-corrective offsets of vertex v for the tile's frames (one pass over posedirs), shaped vertex, skinning weights
__device__ __forceinline__ void kp_vertex_common(const KpBodyDev &B, const float *__restrict__ betas, const float (*spf)[KP_PF], int v,
                                                 float (*po)[3], float *vs, float *wt) {
  for (int fi = 0; fi < KP_FT; fi++) { po[fi][0] = 0.f; po[fi][1] = 0.f; po[fi][2] = 0.f; }
  const float *pd = B.posedirs + (size_t)v * 3;
  const size_t row = (size_t)B.V * 3;
#pragma unroll 3
  for (int k = 0; k < 207; k++) {
    const float p0 = pd[k * row], p1 = pd[k * row + 1], p2 = pd[k * row + 2];
#pragma unroll
    for (int fi = 0; fi < KP_FT; fi++) {
      const float f = spf[fi][k];
      po[fi][0] += f * p0; po[fi][1] += f * p1; po[fi][2] += f * p2;
    }
  }
  for (int c = 0; c < 3; c++) {
    float s = 0.f;
    for (int l = 0; l < 10; l++) s += betas[l] * B.shapedirs[((size_t)v * 3 + c) * 10 + l];
    vs[c] = B.v_template[(size_t)v * 3 + c] + s;
  }
  for (int jn = 0; jn < 24; jn++) wt[jn] = B.lbs_weights[(size_t)v * 24 + jn];
}
__device__ __forceinline__ void kp_blend(const float *wt, const float *A, float *T) {   // T = W A (lbs.py:227-230), joints in order
  for (int c = 0; c < 12; c++) T[c] = 0.f;
  for (int jn = 0; jn < 24; jn++)
    for (int c = 0; c < 12; c++) T[c] += wt[jn] * A[jn * 12 + c];
}

__global__ __launch_bounds__(KP_THREADS) void k_kp_vertex_fwd(KpBodyDev B, const float *__restrict__ betas, const float *__restrict__ transl,
                                                               int F, int n_vb, KpWs w, float *__restrict__ verts) {
  __shared__ float sA[KP_FT][288], spf[KP_FT][KP_PF];
  const int f0 = (int)(blockIdx.x / n_vb) * KP_FT, vb = blockIdx.x % n_vb;   // (tile, vertex block) on one grid axis: neither count is held to 65 535
  kp_load_tile(w, f0, F, sA, spf);
  __syncthreads();
  const int v = vb * KP_THREADS + threadIdx.x;
  if (v >= B.V) return;
  float po[KP_FT][3], vs[3], wt[24];
  kp_vertex_common(B, betas, spf, v, po, vs, wt);
#pragma unroll
  for (int fi = 0; fi < KP_FT; fi++) {
    const int f = f0 + fi;
    if (f >= F) break;
    float T[12];
    kp_blend(wt, sA[fi], T);
    const float vp[3] = {vs[0] + po[fi][0], vs[1] + po[fi][1], vs[2] + po[fi][2]};
    for (int a = 0; a < 3; a++)
      verts[((size_t)f * B.V + v) * 3 + a] = (T[a * 4] * vp[0] + T[a * 4 + 1] * vp[1] + T[a * 4 + 2] * vp[2] + T[a * 4 + 3]) + transl[(size_t)f * 3 + a];
  }
}

// model point m of frame f
__device__ __forceinline__ void kp_point(const KpWs &w, const float *__restrict__ verts, const float *__restrict__ transl,
                                         const int32_t *__restrict__ kp_vertex, int V, size_t f, int m, float *p) {
  if (m < 24)
    for (int a = 0; a < 3; a++) p[a] = w.joints[f * 72 + m * 3 + a] + transl[f * 3 + a];
  else
    for (int a = 0; a < 3; a++) p[a] = verts[(f * V + kp_vertex[m - 24]) * 3 + a];
}
__device__ __forceinline__ void kp_project(const float *__restrict__ P, const float *p, float *q) {
  for (int i = 0; i < 3; i++) q[i] = (P[i * 4] * p[0] + P[i * 4 + 1] * p[1] + P[i * 4 + 2] * p[2]) + P[i * 4 + 3];
}

__global__ __launch_bounds__(KP_THREADS) void k_kp_points(KpWs w, const float *__restrict__ verts, const float *__restrict__ transl,
                                                           const int32_t *__restrict__ kp_vertex, int V, int F, const float *__restrict__ proj,
                                                           const float *__restrict__ keypoints, float threshold, float *__restrict__ points,
                                                           float *__restrict__ uv) {
  const long i = (long)blockIdx.x * KP_THREADS + threadIdx.x;
  if (i >= (long)F * IA_KP_N_POINTS) return;
  const size_t f = i / IA_KP_N_POINTS;
  const int m = (int)(i % IA_KP_N_POINTS);
  float p[3];
  kp_point(w, verts, transl, kp_vertex, V, f, m, p);
  for (int a = 0; a < 3; a++) points[i * 3 + a] = p[a];
  if (m < IA_KP_N_BODY25) {   // this thread also takes BODY_25 point k = m
    float q[3];
    kp_point(w, verts, transl, kp_vertex, V, f, KP_MAP[m], p);
    kp_project(proj, p, q);
    const float u0 = q[0] / q[2], u1 = q[1] / q[2];
    const float *kp = keypoints + (f * IA_KP_N_BODY25 + m) * 3;
    const float dx = kp[0] - u0, dy = kp[1] - u1;
    uv[(f * IA_KP_N_BODY25 + m) * 2] = u0;
    uv[(f * IA_KP_N_BODY25 + m) * 2 + 1] = u1;
    w.e[f * IA_KP_N_BODY25 + m] = kp[2] > threshold ? sqrtf(dx * dx + dy * dy) : 0.f;
  }
}

__device__ __forceinline__ float kp_block_sum(float v, float *s_red) {
  s_red[threadIdx.x] = v;
  __syncthreads();
  for (int s = KP_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) s_red[threadIdx.x] += s_red[threadIdx.x + s];
    __syncthreads();
  }
  const float r = s_red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(KP_THREADS) void k_kp_temporal(const float *__restrict__ verts, long n, int V, float *__restrict__ tpart) {
  __shared__ float s_red[KP_THREADS];
  float acc = 0.f;
  for (long i = (long)blockIdx.x * KP_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * KP_THREADS) {
    const float *a = verts + (size_t)i * 3, *b = a + (size_t)V * 3;
    const float d0 = b[0] - a[0], d1 = b[1] - a[1], d2 = b[2] - a[2];
    acc += sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
  }
  const float r = kp_block_sum(acc, s_red);
  if (threadIdx.x == 0) tpart[blockIdx.x] = r;
}

__global__ __launch_bounds__(KP_THREADS) void k_kp_loss_final(KpWs w, int F, int V, int n_tpart, float *__restrict__ loss) {
  __shared__ float s_red[KP_THREADS];
  float acc = 0.f;
  for (int i = threadIdx.x; i < F * IA_KP_N_BODY25; i += KP_THREADS)
    if (i % IA_KP_N_BODY25 != KP_MIDHIP) acc += w.e[i];
  const float s_kp = kp_block_sum(acc, s_red);
  acc = 0.f;
  for (int i = threadIdx.x; i < n_tpart; i += KP_THREADS) acc += w.tpart[i];
  const float s_t = kp_block_sum(acc, s_red);
  if (threadIdx.x == 0) {
    const float l_kp = s_kp / (24.f * (float)F);
    const float l_t = F > 1 ? s_t / ((float)(F - 1) * (float)V) : 0.f;
    loss[0] = l_kp + l_t; loss[1] = l_kp; loss[2] = l_t;
  }
}

// d loss / d model point: the keypoint term through the projection; zero for points no BODY_25 keypoint maps to, for MidHip, for
// a confidence not above the threshold and for an error of exactly zero
__global__ __launch_bounds__(KP_THREADS) void k_kp_point_grad(KpWs w, const float *__restrict__ verts, const float *__restrict__ transl,
                                                               const int32_t *__restrict__ kp_vertex, int V, int F,
                                                               const float *__restrict__ proj, const float *__restrict__ keypoints,
                                                               float threshold) {
  const long i = (long)blockIdx.x * KP_THREADS + threadIdx.x;
  if (i >= (long)F * IA_KP_N_POINTS) return;
  const size_t f = i / IA_KP_N_POINTS;
  const int m = (int)(i % IA_KP_N_POINTS);
  int k = -1;
  for (int q = 0; q < IA_KP_N_BODY25; q++)
    if (KP_MAP[q] == m) k = q;
  float g[3] = {0.f, 0.f, 0.f};
  if (k >= 0 && k != KP_MIDHIP) {
    const float *kp = keypoints + (f * IA_KP_N_BODY25 + k) * 3;
    if (kp[2] > threshold) {
      float p[3], q[3];
      kp_point(w, verts, transl, kp_vertex, V, f, m, p);
      kp_project(proj, p, q);
      const float u0 = q[0] / q[2], u1 = q[1] / q[2];
      const float dx = u0 - kp[0], dy = u1 - kp[1];
      const float e = sqrtf(dx * dx + dy * dy);
      if (e > 0.f) {
        const float s = 24.f * (float)F;
        const float du0 = dx / e / s, du1 = dy / e / s;
        const float dq0 = du0 / q[2], dq1 = du1 / q[2], dq2 = -(du0 * u0 + du1 * u1) / q[2];
        for (int c = 0; c < 3; c++) g[c] = proj[c] * dq0 + proj[4 + c] * dq1 + proj[8 + c] * dq2;
      }
    }
  }
  for (int c = 0; c < 3; c++) w.dpoint[i * 3 + c] = g[c];
}

__device__ __forceinline__ void kp_unit_diff(const float *a, const float *b, float s, float *acc) {   // acc += s (a - b) / |a - b|, 0 at a == b
  const float d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
  const float n = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
  if (n > 0.f) { acc[0] += s * (d0 / n); acc[1] += s * (d1 / n); acc[2] += s * (d2 / n); }
}

// GIVEN: `verts` holds the caller's d vert [F,V,3] (ia_sil_body_bwd) and kp_vertex is not read
template <bool GIVEN>
__global__ __launch_bounds__(KP_THREADS) void k_kp_vertex_bwd(KpBodyDev B, const float *__restrict__ betas, int F, int n_vb, KpWs w,
                                                               const float *__restrict__ verts, const int32_t *__restrict__ kp_vertex) {
  __shared__ float sA[KP_FT][288], spf[KP_FT][KP_PF];
  __shared__ float sdv[KP_FT][KP_THREADS][3], svp[KP_FT][KP_THREADS][3], sdvp[KP_FT][KP_THREADS][3];
  __shared__ float sdpt[KP_FT][IA_KP_N_VERTEX][3];
  __shared__ int skv[IA_KP_N_VERTEX];
  const int tid = threadIdx.x, f0 = (int)(blockIdx.x / n_vb) * KP_FT, vb = blockIdx.x % n_vb, v0 = vb * KP_THREADS, V = B.V;
  kp_load_tile(w, f0, F, sA, spf);
  if (!GIVEN) {
    if (tid < IA_KP_N_VERTEX) skv[tid] = kp_vertex[tid];
    for (int i = tid; i < KP_FT * IA_KP_N_VERTEX * 3; i += KP_THREADS) {
      const int fi = i / (IA_KP_N_VERTEX * 3), r = i % (IA_KP_N_VERTEX * 3);
      sdpt[fi][r / 3][r % 3] = f0 + fi < F ? w.dpoint[((size_t)(f0 + fi) * IA_KP_N_POINTS + 24) * 3 + r] : 0.f;
    }
  }
  __syncthreads();
  // phase A, one thread per vertex: d vert, vs + po and T.R^T d vert of the tile's frames into LDS
  const int v = v0 + tid;
  if (v < V) {
    float po[KP_FT][3], vs[3], wt[24];
    kp_vertex_common(B, betas, spf, v, po, vs, wt);
    const float gt = F > 1 ? 1.f / ((float)(F - 1) * (float)V) : 0.f;
#pragma unroll
    for (int fi = 0; fi < KP_FT; fi++) {
      const int f = f0 + fi;
      float dv[3] = {0.f, 0.f, 0.f}, vp[3] = {0.f, 0.f, 0.f}, dvp[3] = {0.f, 0.f, 0.f};
      if (f < F) {
        const float *x = verts + ((size_t)f * V + v) * 3;
        if (GIVEN) {
          dv[0] = x[0]; dv[1] = x[1]; dv[2] = x[2];
        } else {
          if (f > 0) kp_unit_diff(x, x - (size_t)V * 3, gt, dv);
          if (f < F - 1) kp_unit_diff(x, x + (size_t)V * 3, gt, dv);   // -(x1 - x) / |x1 - x| = (x - x1) / |x - x1|
          for (int m = 0; m < IA_KP_N_VERTEX; m++)
            if (skv[m] == v) { dv[0] += sdpt[fi][m][0]; dv[1] += sdpt[fi][m][1]; dv[2] += sdpt[fi][m][2]; }
        }
        float T[12];
        kp_blend(wt, sA[fi], T);
        for (int b = 0; b < 3; b++) {
          vp[b] = vs[b] + po[fi][b];
          dvp[b] = T[b] * dv[0] + T[4 + b] * dv[1] + T[8 + b] * dv[2];
        }
      }
      for (int c = 0; c < 3; c++) { sdv[fi][tid][c] = dv[c]; svp[fi][tid][c] = vp[c]; sdvp[fi][tid][c] = dvp[c]; }
    }
  } else {
    for (int fi = 0; fi < KP_FT; fi++)
      for (int c = 0; c < 3; c++) { sdv[fi][tid][c] = 0.f; svp[fi][tid][c] = 0.f; sdvp[fi][tid][c] = 0.f; }
  }
  __syncthreads();
  // phase B, one thread per output: sums over the block's vertices in vertex order
  const int nv = V - v0 < KP_THREADS ? V - v0 : KP_THREADS;
  const size_t row = (size_t)V * 3;
  for (int o = tid; o < KP_NOUT; o += KP_THREADS) {
    float acc[KP_FT];
    for (int fi = 0; fi < KP_FT; fi++) acc[fi] = 0.f;
    if (o < KP_O_PF) {             // d A_j = sum_v w_vj [d vert (vs + po)^T | d vert]
      const int jn = o / 12, a = (o % 12) >> 2, b = o & 3;
      for (int q = 0; q < nv; q++) {
        const float wv = B.lbs_weights[(size_t)(v0 + q) * 24 + jn];
#pragma unroll
        for (int fi = 0; fi < KP_FT; fi++) acc[fi] += wv * (b < 3 ? sdv[fi][q][a] * svp[fi][q][b] : sdv[fi][q][a]);
      }
    } else if (o < KP_O_BETA) {    // d pf[k] = sum_v posedirs[k, v, :] . d po[v]
      const float *pd = B.posedirs + (size_t)(o - KP_O_PF) * row + (size_t)v0 * 3;
      for (int q = 0; q < nv * 3; q++) {
        const float p = pd[q];
#pragma unroll
        for (int fi = 0; fi < KP_FT; fi++) acc[fi] += p * sdvp[fi][q / 3][q % 3];
      }
    } else if (o < KP_O_TR) {      // d betas through the shape blend
      const float *sd = B.shapedirs + (size_t)v0 * 30 + (o - KP_O_BETA);
      for (int q = 0; q < nv * 3; q++) {
        const float p = sd[(size_t)q * 10];
#pragma unroll
        for (int fi = 0; fi < KP_FT; fi++) acc[fi] += p * sdvp[fi][q / 3][q % 3];
      }
    } else {                       // d transl = sum_v d vert
      for (int q = 0; q < nv; q++)
#pragma unroll
        for (int fi = 0; fi < KP_FT; fi++) acc[fi] += sdv[fi][q][o - KP_O_TR];
    }
    for (int fi = 0; fi < KP_FT; fi++)
      if (f0 + fi < F) w.part[((size_t)(f0 + fi) * n_vb + vb) * KP_NOUT + o] = acc[fi];
  }
}

__global__ __launch_bounds__(KP_THREADS) void k_kp_reduce_v(KpWs w, int F, int n_vb) {
  const long i = (long)blockIdx.x * KP_THREADS + threadIdx.x;
  if (i >= (long)F * KP_NOUT) return;
  const size_t f = i / KP_NOUT, o = i % KP_NOUT;
  float acc = 0.f;
  for (int b = 0; b < n_vb; b++) acc += w.part[(f * n_vb + b) * KP_NOUT + o];
  w.red[i] = acc;
}

__global__ void k_kp_chain_bwd(KpBodyDev B, const float *__restrict__ betas, const float *__restrict__ pose, KpWs w,
                               float *__restrict__ d_pose, float *__restrict__ d_transl) {
  __shared__ float R[24][9], Jn[24][3], G[24][12];
  __shared__ float dA[24][12], dRG[24][9], dg[24][3], dRl[24][9], dJ[24][3], dGt[24][3];
  __shared__ int par[24];
  const int j = threadIdx.x;
  const size_t f = blockIdx.x;
  const float *red = w.red + f * KP_NOUT;
  Rod rod;
  if (j < 24) {
    par[j] = B.parents[j];
    for (int c = 0; c < 3; c++) {
      float v = B.J0[j * 3 + c];
      for (int l = 0; l < 10; l++) v += B.JS[(j * 3 + c) * 10 + l] * betas[l];
      Jn[j][c] = v;
      dJ[j][c] = 0.f;
      dGt[j][c] = w.dpoint[(f * IA_KP_N_POINTS + j) * 3 + c];
    }
    rodrigues(pose + f * 72 + j * 3, rod);
    for (int a = 0; a < 9; a++) R[j][a] = rod.R[a];
    for (int c = 0; c < 12; c++) dA[j][c] = red[j * 12 + c];
  }
  __syncthreads();
  chain_forward(R, Jn, par, G, j);
  if (j < 3 && d_transl) {   // transl enters every vertex and every joint
    float v = red[KP_O_TR + j];
    for (int i = 0; i < 24; i++) v += dGt[i][j];
    d_transl[f * 3 + j] = v;
  }
  chain_backward(dA, R, G, Jn, par, dRG, dg, dRl, dJ, j, dGt);
  if (j < 24 && d_pose) {
    float dR[9];
    for (int a = 0; a < 9; a++) dR[a] = dRl[j][a] + (j >= 1 ? red[KP_O_PF + (j - 1) * 9 + a] : 0.f);
    float dth[3];
    rodrigues_bwd(pose + f * 72 + j * 3, rod, dR, dth);
    for (int a = 0; a < 3; a++) d_pose[f * 72 + j * 3 + a] = dth[a];
  }
  __syncthreads();
  if (j < 10) {   // J = J0 + JS beta, vs = v_template + shapedirs beta
    float v = 0.f;
    for (int i = 0; i < 24; i++)
      for (int c = 0; c < 3; c++) v += B.JS[(i * 3 + c) * 10 + j] * dJ[i][c];
    w.dbf[f * 10 + j] = v + red[KP_O_BETA + j];
  }
}

__global__ void k_kp_reduce_f(KpWs w, int F, float *__restrict__ d_betas) {
  const int j = threadIdx.x;
  if (j >= 10) return;
  float acc = 0.f;
  for (int f = 0; f < F; f++) acc += w.dbf[(size_t)f * 10 + j];
  d_betas[j] = acc;
}

static int kp_make_body(const ia_smpl_body *b, KpBodyDev *o) {
  if (!b || !b->v_template || !b->shapedirs || !b->posedirs || !b->lbs_weights || !b->J0 || !b->JS || !b->parents) return 1;
  o->v_template = b->v_template; o->shapedirs = b->shapedirs; o->posedirs = b->posedirs; o->lbs_weights = b->lbs_weights;
  o->J0 = b->J0; o->JS = b->JS; o->parents = b->parents; o->V = b->n_verts;
  return 0;
}

// the first kernel of either entry: kp_vertex checked where it lives; the host reads the flag back before it launches anything else
static int kp_check_vertices(const int32_t *kp_vertex, int V, int32_t *flag, hipStream_t s, const char *who) {
  hipLaunchKernelGGL(k_kp_check, dim3(1), dim3(64), 0, s, kp_vertex, V, flag);
  IA_LAUNCH_CHECK("k_kp_check");
  int32_t bad = 1;
  hipError_t e = hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return ia_set_error(IA_ERR_LAUNCH, "%s: reading the kp_vertex check back: %s", who, hipGetErrorString(e));
  IA_CHECK_ARG(bad == 0, "%s: a kp_vertex entry is outside [0, n_verts = %d)", who, V);
  return IA_OK;
}

#define KP_CHECK_COMMON(who)                                                                                                   \
  KpBodyDev B;                                                                                                                 \
  IA_CHECK_ARG(kp_make_body(body, &B) == 0, who ": incomplete body model");                                                   \
  IA_CHECK_ARG(n_frames >= 1, who ": n_frames = %d < 1", n_frames);                                                           \
  IA_CHECK_ARG(B.V >= 1, who ": body with n_verts = %d < 1", B.V);                                                            \
  IA_CHECK_ARG(kp_sizes_ok(n_frames, B.V), who ": n_frames * n_verts * 3 = %lld does not fit 31 bits", (long long)n_frames * B.V * 3); \
  IA_CHECK_ARG(betas && pose && transl && proj && keypoints && kp_vertex && ws, who ": null pointer");                         \
  IA_CHECK_ARG(ws_bytes >= ia_kp_workspace_bytes(n_frames, B.V), who ": workspace too small");                                 \
  hipStream_t s = (hipStream_t)stream;                                                                                         \
  const int F = n_frames;                                                                                                      \
  KpWs w = kp_carve(ws, F, B.V);                                                                                               \
  {                                                                                                                            \
    const int rc = kp_check_vertices(kp_vertex, B.V, w.flag, s, who);                                                          \
    if (rc != IA_OK) return rc;                                                                                                \
  }

extern "C" int ia_kp_loss_fwd(const ia_smpl_body *body, const float *betas, const float *pose, const float *transl, int n_frames,
                              const float *proj, const float *keypoints, float threshold, const int32_t *kp_vertex, float *verts,
                              float *points, float *uv, float *loss, void *ws, size_t ws_bytes, void *stream) {
  KP_CHECK_COMMON("ia_kp_loss_fwd")
  if (!verts) verts = w.verts;
  if (!points) points = w.points;
  if (!uv) uv = w.uv;
  const int n_vb = ia_div_up(B.V, KP_THREADS);
  hipLaunchKernelGGL(k_kp_chain_fwd, dim3(F), dim3(64), 0, s, B, betas, pose, w);
  IA_LAUNCH_CHECK("k_kp_chain_fwd");
  hipLaunchKernelGGL(k_kp_vertex_fwd, dim3((unsigned)((long)n_vb * ia_div_up(F, KP_FT))), dim3(KP_THREADS), 0, s, B, betas, transl, F, n_vb, w, verts);
  IA_LAUNCH_CHECK("k_kp_vertex_fwd");
  hipLaunchKernelGGL(k_kp_points, dim3(ia_div_up((long)F * IA_KP_N_POINTS, KP_THREADS)), dim3(KP_THREADS), 0, s, w, verts, transl, kp_vertex,
                     B.V, F, proj, keypoints, threshold, points, uv);
  IA_LAUNCH_CHECK("k_kp_points");
  if (loss) {
    const long n = (long)(F - 1) * B.V;
    const int n_tpart = n > 0 ? (ia_div_up(n, KP_THREADS) < KP_TBLOCKS ? ia_div_up(n, KP_THREADS) : KP_TBLOCKS) : 0;
    if (n_tpart > 0) {
      hipLaunchKernelGGL(k_kp_temporal, dim3(n_tpart), dim3(KP_THREADS), 0, s, verts, n, B.V, w.tpart);
      IA_LAUNCH_CHECK("k_kp_temporal");
    }
    hipLaunchKernelGGL(k_kp_loss_final, dim3(1), dim3(KP_THREADS), 0, s, w, F, B.V, n_tpart, loss);
    IA_LAUNCH_CHECK("k_kp_loss_final");
  }
  return IA_OK;
}

extern "C" int ia_kp_loss_bwd(const ia_smpl_body *body, const float *betas, const float *pose, const float *transl, int n_frames,
                              const float *proj, const float *keypoints, float threshold, const int32_t *kp_vertex, const float *verts,
                              float *d_betas, float *d_pose, float *d_transl, void *ws, size_t ws_bytes, void *stream) {
  IA_CHECK_ARG(verts, "ia_kp_loss_bwd: null verts");
  KP_CHECK_COMMON("ia_kp_loss_bwd")
  const int n_vb = ia_div_up(B.V, KP_THREADS);
  hipLaunchKernelGGL(k_kp_chain_fwd, dim3(F), dim3(64), 0, s, B, betas, pose, w);
  IA_LAUNCH_CHECK("k_kp_chain_fwd");
  hipLaunchKernelGGL(k_kp_point_grad, dim3(ia_div_up((long)F * IA_KP_N_POINTS, KP_THREADS)), dim3(KP_THREADS), 0, s, w, verts, transl,
                     kp_vertex, B.V, F, proj, keypoints, threshold);
  IA_LAUNCH_CHECK("k_kp_point_grad");
  hipLaunchKernelGGL(k_kp_vertex_bwd<false>, dim3((unsigned)((long)n_vb * ia_div_up(F, KP_FT))), dim3(KP_THREADS), 0, s, B, betas, F, n_vb, w, verts, kp_vertex);
  IA_LAUNCH_CHECK("k_kp_vertex_bwd");
  hipLaunchKernelGGL(k_kp_reduce_v, dim3(ia_div_up((long)F * KP_NOUT, KP_THREADS)), dim3(KP_THREADS), 0, s, w, F, n_vb);
  IA_LAUNCH_CHECK("k_kp_reduce_v");
  hipLaunchKernelGGL(k_kp_chain_bwd, dim3(F), dim3(64), 0, s, B, betas, pose, w, d_pose, d_transl);
  IA_LAUNCH_CHECK("k_kp_chain_bwd");
  if (d_betas) {
    hipLaunchKernelGGL(k_kp_reduce_f, dim3(1), dim3(64), 0, s, w, F, d_betas);
    IA_LAUNCH_CHECK("k_kp_reduce_f");
  }
  return IA_OK;
}

// ---- the same backward for a vertex cotangent of the caller's (include/instantavatar_hip_silhouette.h) ---------------------------
extern "C" size_t ia_sil_body_workspace_bytes(int n_frames, int n_verts) { return ia_kp_workspace_bytes(n_frames, n_verts); }

extern "C" int ia_sil_body_bwd(const ia_smpl_body *body, const float *betas, const float *pose, const float *transl, int n_frames,
                               const float *d_verts, float *d_betas, float *d_pose, float *d_transl, void *ws, size_t ws_bytes, void *stream) {
  KpBodyDev B;
  IA_CHECK_ARG(kp_make_body(body, &B) == 0, "ia_sil_body_bwd: incomplete body model");
  IA_CHECK_ARG(n_frames >= 1, "ia_sil_body_bwd: n_frames = %d < 1", n_frames);
  IA_CHECK_ARG(B.V >= 1, "ia_sil_body_bwd: body with n_verts = %d < 1", B.V);
  IA_CHECK_ARG(kp_sizes_ok(n_frames, B.V), "ia_sil_body_bwd: n_frames * n_verts * 3 = %lld does not fit 31 bits", (long long)n_frames * B.V * 3);
  IA_CHECK_ARG(betas && pose && transl && d_verts && ws, "ia_sil_body_bwd: null pointer");
  IA_CHECK_ARG(ws_bytes >= ia_kp_workspace_bytes(n_frames, B.V), "ia_sil_body_bwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int F = n_frames, n_vb = ia_div_up(B.V, KP_THREADS);
  KpWs w = kp_carve(ws, F, B.V);
  hipLaunchKernelGGL(k_kp_chain_fwd, dim3(F), dim3(64), 0, s, B, betas, pose, w);
  IA_LAUNCH_CHECK("k_kp_chain_fwd");
  ia_zero_fill(w.dpoint, (size_t)F * IA_KP_N_POINTS * 3 * sizeof(float), s);   // no cotangent of the joints themselves
  IA_LAUNCH_CHECK("k_zero_words");
  hipLaunchKernelGGL(k_kp_vertex_bwd<true>, dim3((unsigned)((long)n_vb * ia_div_up(F, KP_FT))), dim3(KP_THREADS), 0, s, B, betas, F, n_vb, w, d_verts,
                     (const int32_t *)nullptr);
  IA_LAUNCH_CHECK("k_kp_vertex_bwd");
  hipLaunchKernelGGL(k_kp_reduce_v, dim3(ia_div_up((long)F * KP_NOUT, KP_THREADS)), dim3(KP_THREADS), 0, s, w, F, n_vb);
  IA_LAUNCH_CHECK("k_kp_reduce_v");
  hipLaunchKernelGGL(k_kp_chain_bwd, dim3(F), dim3(64), 0, s, B, betas, pose, w, d_pose, d_transl);
  IA_LAUNCH_CHECK("k_kp_chain_bwd");
  if (d_betas) {
    hipLaunchKernelGGL(k_kp_reduce_f, dim3(1), dim3(64), 0, s, w, F, d_betas);
    IA_LAUNCH_CHECK("k_kp_reduce_f");
  }
  return IA_OK;
}
