// ia_rig.hip -- the standard rig of the canonical mesh (no counterpart in the reference, which never exports geometry):
//   per-vertex joint indices and weights: the K largest of the 24 trilinear skinning weights, renormalised   (ia_rig_weights)
//   bone matrices, joint quaternions and root translations of a whole pose track, one workgroup per frame     (ia_rig_track)
//   linear-blend skinning of the mesh over every frame of the track in one launch                             (ia_rig_skin)
// The definitions are stated in DESIGN.md section 4 ("rigged export") and in include/instantavatar_hip_rig.h.  The weight gather
// restates ia_snarf.hip's id_sample_weights (same corner order, same fmaf chain) instead of sharing it through a header: that
// translation unit's device code stays what the committed counter summaries were collected on.  Nothing here synchronises,
// allocates, reads on the host or uses an atomic, so two calls on the same input give the same bytes.
#include "ia_common.h"
#include "ia_smpl_dev.h"
#include "../../include/instantavatar_hip_rig.h"

#define IA_RIG_THREADS 256
// ia_rig_skin: frames whose bone matrices a workgroup holds in LDS between two barriers (24 x 12 floats each: 18 KiB per workgroup,
// eight workgroups per CU), and the number of workgroups up to which the frames of a vertex tile are split over blockIdx.y.  Measured
// on the synthetic model's full mesh (108 518 vertices, 200 frames, K = 4 / 8; two rounds, run to run +-10 %): 1 536 workgroups
// 0.134 / 0.166 ms, 2 048: 0.128-0.144 / 0.164-0.169, 8 192: 0.110-0.124 / 0.158-0.167, 32 768: 0.113-0.120 / 0.218-0.221 (three frames
// per workgroup no longer pay for loading its vertices); stages of 8 or 4 frames instead of 16 change nothing.
#define IA_RIG_FRAMES 16
#define IA_RIG_TARGET_BLOCKS 8192

namespace {

__device__ __forceinline__ float rig_border_index(float g, int size) {
  float c = ((g + 1.f) / 2) * (size - 1);          // align_corners = true
  return fminf(fmaxf(c, 0.f), (float)(size - 1));   // padding_mode = "border"
}

// the 24 skinning weights at x: trilinear, align_corners, border padding (ForwardDeformer.query_weights); w is zeroed by the caller.
// CL: voxel_w is channel-last [D,H,W,24], six 16-byte loads per corner
template <bool CL>
__device__ __forceinline__ void rig_sample_weights(const float *__restrict__ voxel_w, const SnarfGridDev &g, float x0, float x1, float x2,
                                                   float *__restrict__ w) {
  const long vol = (long)g.D * g.H * g.W;
  const float ix = rig_border_index(g.scl[0] * (x0 + g.off[0]), g.W);
  const float iy = rig_border_index(g.scl[1] * (x1 + g.off[1]), g.H);
  const float iz = rig_border_index(g.scl[2] * (x2 + g.off[2]), g.D);
  const int xa = (int)floorf(ix), ya = (int)floorf(iy), za = (int)floorf(iz);      // in [0, size - 1] after the clamp
  const float fx = ix - xa, fy = iy - ya, fz = iz - za;
#pragma unroll
  for (int cz = 0; cz < 2; cz++)
#pragma unroll
    for (int cy = 0; cy < 2; cy++)
#pragma unroll
      for (int cx = 0; cx < 2; cx++) {
        const int xx = xa + cx, yy = ya + cy, zz = za + cz;
        if (xx >= g.W || yy >= g.H || zz >= g.D) continue;  // only at the clamped border, weight 0
        const float wt = (cx ? fx : 1.f - fx) * (cy ? fy : 1.f - fy) * (cz ? fz : 1.f - fz);
        if (CL) {
          const float4 *p4 = reinterpret_cast<const float4 *>(voxel_w + (((long)zz * g.H + yy) * g.W + xx) * 24);
#pragma unroll
          for (int q = 0; q < 6; q++) {
            const float4 v = p4[q];
            w[4 * q] = __builtin_fmaf(wt, v.x, w[4 * q]); w[4 * q + 1] = __builtin_fmaf(wt, v.y, w[4 * q + 1]);
            w[4 * q + 2] = __builtin_fmaf(wt, v.z, w[4 * q + 2]); w[4 * q + 3] = __builtin_fmaf(wt, v.w, w[4 * q + 3]);
          }
        } else {
          const float *p = voxel_w + ((long)zz * g.H + yy) * g.W + xx;
#pragma unroll
          for (int k = 0; k < 24; k++) w[k] = __builtin_fmaf(wt, p[(long)k * vol], w[k]);
        }
      }
}

// One thread per point.  Every array index below is a compile-time constant after unrolling (the selection is 24 x 24 compare /
// select steps on registers, K being the same in every lane), so nothing lives in scratch.
template <bool CL>
__global__ __launch_bounds__(IA_RIG_THREADS) void k_rig_weights(const float *__restrict__ xc, int n, const float *__restrict__ voxel_w,
                                                                SnarfGridDev g, int K, uint8_t *__restrict__ joints,
                                                                float *__restrict__ weights, float *__restrict__ full) {
  const int p = blockIdx.x * IA_RIG_THREADS + threadIdx.x;
  if (p >= n) return;
  const float x0 = xc[(size_t)p * 3], x1 = xc[(size_t)p * 3 + 1], x2 = xc[(size_t)p * 3 + 2];
  const bool finite = __builtin_isfinite(x0) && __builtin_isfinite(x1) && __builtin_isfinite(x2);
  float w[24];
#pragma unroll
  for (int j = 0; j < 24; j++) w[j] = 0.f;
  if (finite) rig_sample_weights<CL>(voxel_w, g, x0, x1, x2, w);
  if (full) {
#pragma unroll
    for (int j = 0; j < 24; j++) full[(size_t)p * 24 + j] = w[j];
  }
  float sw[24];
  int sj[24];
  unsigned used = 0u;
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < 24; k++) {
    sw[k] = 0.f;
    sj[k] = 0;
    if (k < K) {
      float best = -INFINITY;
      int bj = -1;
#pragma unroll
      for (int j = 0; j < 24; j++) {
        const bool take = !((used >> j) & 1u) && w[j] > best;      // strict: a tie keeps the lower joint; NaN never compares greater
        best = take ? w[j] : best;
        bj = take ? j : bj;
      }
      if (bj >= 0) {
        used |= 1u << bj;
        sw[k] = best;
        sj[k] = best == 0.f ? 0 : bj;
      }
      sum += sw[k];
    }
  }
  const bool ok = finite && sum != 0.f && __builtin_isfinite(sum);
#pragma unroll
  for (int k = 0; k < 24; k++)
    if (k < K) {
      joints[(size_t)p * K + k] = (uint8_t)(ok ? sj[k] : 0);
      weights[(size_t)p * K + k] = ok ? sw[k] / sum : (k == 0 ? 1.f : 0.f);
    }
}

// One workgroup of 64 threads per frame; lanes 0..23 own one joint each, the chain runs through ia_smpl_dev.h's chain_forward.
__global__ __launch_bounds__(64) void k_rig_track(const float *__restrict__ joints_rest, const int32_t *__restrict__ parents,
                                                  const float *__restrict__ poses, const float *__restrict__ transl,
                                                  const float *__restrict__ tfs_inv_t, float *__restrict__ bones,
                                                  float *__restrict__ quat, float *__restrict__ root_t) {
  __shared__ float s_R[24][9];
  __shared__ float s_J[24][3];
  __shared__ float s_G[24][12];
  __shared__ int s_par[24];
  const int j = threadIdx.x;
  const size_t f = blockIdx.x;
  if (j < 24) {
    s_par[j] = parents[j];
    for (int a = 0; a < 3; a++) s_J[j][a] = joints_rest[j * 3 + a];
    const float *th = poses + f * 72 + j * 3;
    Rod r;
    rodrigues(th, r);
    for (int a = 0; a < 9; a++) s_R[j][a] = r.R[a];
    if (quat) {
      const float h = 0.5f * r.ang;
      const float sh = sinf(h), ch = cosf(h);
      const float q0 = (th[0] / r.ang) * sh, q1 = (th[1] / r.ang) * sh, q2 = (th[2] / r.ang) * sh;
      const float len = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + ch * ch);
      float *q = quat + (f * 24 + j) * 4;
      q[0] = q0 / len; q[1] = q1 / len; q[2] = q2 / len; q[3] = ch / len;
    }
  }
  __syncthreads();
  chain_forward(s_R, s_J, s_par, s_G, j);      // (ends in a barrier)
  const float t0 = transl ? transl[f * 3] : 0.f, t1 = transl ? transl[f * 3 + 1] : 0.f, t2 = transl ? transl[f * 3 + 2] : 0.f;
  if (j < 3 && root_t) root_t[f * 3 + j] = s_J[0][j] + (j == 0 ? t0 : j == 1 ? t1 : t2);
  if (j < 24) {
    // A_j = T(transl) G_j T(-J_j), then B_j = A_j . tfs_inv_t_j with the summation order of ia_smpl_tfs's products
    float A[16], B[16];
    const float tr[3] = {t0, t1, t2};
    for (int a = 0; a < 3; a++) {
      const float t = s_G[j][a * 4] * s_J[j][0] + s_G[j][a * 4 + 1] * s_J[j][1] + s_G[j][a * 4 + 2] * s_J[j][2];
      for (int b = 0; b < 3; b++) A[a * 4 + b] = s_G[j][a * 4 + b];
      A[a * 4 + 3] = (s_G[j][a * 4 + 3] - t) + tr[a];
    }
    A[12] = 0.f; A[13] = 0.f; A[14] = 0.f; A[15] = 1.f;
    const float *T = tfs_inv_t + j * 16;
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 4; b++) {
        float s = 0.f;
        for (int k = 0; k < 4; k++) s += A[a * 4 + k] * T[k * 4 + b];
        B[a * 4 + b] = s;
      }
    B[12] = 0.f; B[13] = 0.f; B[14] = 0.f; B[15] = 1.f;
    float *out = bones + (f * 24 + j) * 16;
    for (int k = 0; k < 16; k++) out[k] = B[k];
  }
}

// The hot path.  A workgroup owns IA_RIG_THREADS vertices (one per thread: position, normal, indices and weights stay in registers)
// and a range of frames; it stages the bone matrices of IA_RIG_FRAMES frames in LDS (rows 0..2: 24 x 12 floats per frame, 16-byte
// loads), and every thread then reads the three float4 rows of each of its K joints per frame (48-byte records: distinct joints fall
// into distinct banks of a ds_read_b128 lane group but for the pairs 16 apart, equal joints broadcast) and stores 12 or 24 bytes next
// to its neighbours' -- a wave writes 768 contiguous bytes per frame and output.  Per frame and vertex that is 3 K LDS reads and
// 12 K + 18 fmaf against 24 bytes stored.  KP: K rounded up to the register arrays' size (4, 8 or 24).
template <int KP, bool NRM>
__global__ __launch_bounds__(IA_RIG_THREADS) void k_rig_skin(const float *__restrict__ verts, const float *__restrict__ normals, int n,
                                                             const uint8_t *__restrict__ joints, const float *__restrict__ weights, int K,
                                                             const float *__restrict__ bones, int F, int frames_per_block,
                                                             float *__restrict__ out_verts, float *__restrict__ out_normals) {
  __shared__ float4 s_b[IA_RIG_FRAMES][24][3];
  const int v = blockIdx.x * IA_RIG_THREADS + threadIdx.x;
  const bool live = v < n;
  float x[3] = {0.f, 0.f, 0.f}, nn[3] = {0.f, 0.f, 0.f}, w[KP];
  int jn[KP];
#pragma unroll
  for (int k = 0; k < KP; k++) {
    w[k] = 0.f;
    jn[k] = 0;
  }
  if (live) {
#pragma unroll
    for (int a = 0; a < 3; a++) x[a] = verts[(size_t)v * 3 + a];
    if (NRM) {
#pragma unroll
      for (int a = 0; a < 3; a++) nn[a] = normals[(size_t)v * 3 + a];
    }
#pragma unroll
    for (int k = 0; k < KP; k++)
      if (k < K) {
        w[k] = weights[(size_t)v * K + k];
        jn[k] = min((int)joints[(size_t)v * K + k], 23);
      }
  }
  const int f_begin = blockIdx.y * frames_per_block, f_end = min(F, f_begin + frames_per_block);
  for (int f0 = f_begin; f0 < f_end; f0 += IA_RIG_FRAMES) {
    const int nf = min(IA_RIG_FRAMES, f_end - f0);
    __syncthreads();                                                  // the previous frames' reads are done
    for (int i = threadIdx.x; i < nf * 72; i += IA_RIG_THREADS) {
      const int fl = i / 72, r = i - fl * 72, j = r / 3, row = r - j * 3;
      s_b[fl][j][row] = *reinterpret_cast<const float4 *>(bones + ((size_t)(f0 + fl) * 24 + j) * 16 + row * 4);
    }
    __syncthreads();
    if (!live) continue;
    for (int fl = 0; fl < nf; fl++) {
      float M[12];
#pragma unroll
      for (int q = 0; q < 12; q++) M[q] = 0.f;
#pragma unroll
      for (int k = 0; k < KP; k++)
        if (k < K) {
#pragma unroll
          for (int row = 0; row < 3; row++) {
            const float4 b = s_b[fl][jn[k]][row];
            M[4 * row] = __builtin_fmaf(w[k], b.x, M[4 * row]);
            M[4 * row + 1] = __builtin_fmaf(w[k], b.y, M[4 * row + 1]);
            M[4 * row + 2] = __builtin_fmaf(w[k], b.z, M[4 * row + 2]);
            M[4 * row + 3] = __builtin_fmaf(w[k], b.w, M[4 * row + 3]);
          }
        }
      const size_t o = ((size_t)(f0 + fl) * n + v) * 3;
#pragma unroll
      for (int a = 0; a < 3; a++) out_verts[o + a] = IA_DOT3(M[4 * a], x[0], M[4 * a + 1], x[1], M[4 * a + 2], x[2]) + M[4 * a + 3];
      if (NRM) {
        float m[3];
#pragma unroll
        for (int a = 0; a < 3; a++) m[a] = IA_DOT3(M[4 * a], nn[0], M[4 * a + 1], nn[1], M[4 * a + 2], nn[2]);
        const float len = sqrtf(IA_DOT3(m[0], m[0], m[1], m[1], m[2], m[2]));
        const bool ok = len > 0.f && __builtin_isfinite(len);
#pragma unroll
        for (int a = 0; a < 3; a++) out_normals[o + a] = ok ? m[a] / len : 0.f;
      }
    }
  }
}

template <int KP>
void rig_launch_skin(bool nrm, dim3 grid, hipStream_t s, const float *verts, const float *normals, int n, const uint8_t *joints,
                     const float *weights, int K, const float *bones, int F, int fpb, float *out_verts, float *out_normals) {
  if (nrm)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rig_skin<KP, true>), grid, dim3(IA_RIG_THREADS), 0, s, verts, normals, n, joints, weights, K, bones,
                       F, fpb, out_verts, out_normals);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rig_skin<KP, false>), grid, dim3(IA_RIG_THREADS), 0, s, verts, normals, n, joints, weights, K, bones,
                       F, fpb, out_verts, out_normals);
}

}  // namespace

extern "C" int ia_rig_weights(const float *xc, int n, const float *voxel_w, int channel_last, const ia_snarf_grid *grid, int K,
                              uint8_t *joints, float *weights, float *full, void *stream) {
  IA_CHECK_ARG(n >= 0, "ia_rig_weights: n = %d < 0", n);
  IA_CHECK_ARG(K >= 1 && K <= IA_RIG_MAX_INFLUENCES, "ia_rig_weights: K = %d outside [1, %d]", K, IA_RIG_MAX_INFLUENCES);
  if (n == 0) return IA_OK;
  IA_CHECK_ARG(xc && voxel_w && grid && joints && weights, "ia_rig_weights: null pointer");
  IA_CHECK_ARG(grid->D > 0 && grid->H > 0 && grid->W > 0, "ia_rig_weights: bad grid %d x %d x %d", grid->D, grid->H, grid->W);
  IA_CHECK_ARG(!channel_last || (reinterpret_cast<uintptr_t>(voxel_w) & 15) == 0,
               "ia_rig_weights: the channel-last weight volume must be 16-byte aligned");
  const dim3 blocks(ia_div_up(n, IA_RIG_THREADS)), threads(IA_RIG_THREADS);
  const SnarfGridDev g = ia_make_grid_dev(grid);
  if (channel_last)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rig_weights<true>), blocks, threads, 0, (hipStream_t)stream, xc, n, voxel_w, g, K, joints, weights, full);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rig_weights<false>), blocks, threads, 0, (hipStream_t)stream, xc, n, voxel_w, g, K, joints, weights, full);
  IA_LAUNCH_CHECK("k_rig_weights");
  return IA_OK;
}

extern "C" int ia_rig_track(const float *joints_rest, const int32_t *parents, const float *poses, const float *transl,
                            const float *tfs_inv_t, int F, float *bones, float *quat, float *root_t, void *stream) {
  IA_CHECK_ARG(F >= 0, "ia_rig_track: F = %d < 0", F);
  if (F == 0) return IA_OK;
  IA_CHECK_ARG(joints_rest && parents && poses && tfs_inv_t && bones, "ia_rig_track: null pointer");
  hipLaunchKernelGGL(k_rig_track, dim3(F), dim3(64), 0, (hipStream_t)stream, joints_rest, parents, poses, transl, tfs_inv_t, bones, quat,
                     root_t);
  IA_LAUNCH_CHECK("k_rig_track");
  return IA_OK;
}

extern "C" int ia_rig_skin(const float *verts, const float *normals, int n, const uint8_t *joints, const float *weights, int K,
                           const float *bones, int F, float *out_verts, float *out_normals, void *stream) {
  IA_CHECK_ARG(n >= 0, "ia_rig_skin: n = %d < 0", n);
  IA_CHECK_ARG(F >= 0, "ia_rig_skin: F = %d < 0", F);
  IA_CHECK_ARG(K >= 1 && K <= IA_RIG_MAX_INFLUENCES, "ia_rig_skin: K = %d outside [1, %d]", K, IA_RIG_MAX_INFLUENCES);
  IA_CHECK_ARG((normals == nullptr) == (out_normals == nullptr), "ia_rig_skin: normals and out_normals are given together or not at all");
  if (n == 0 || F == 0) return IA_OK;
  IA_CHECK_ARG(verts && joints && weights && bones && out_verts, "ia_rig_skin: null pointer");
  IA_CHECK_ARG((reinterpret_cast<uintptr_t>(bones) & 15) == 0, "ia_rig_skin: the bone matrices must be 16-byte aligned");
  // the frames of a vertex tile are split evenly over blockIdx.y until the launch has IA_RIG_TARGET_BLOCKS workgroups
  const int vblocks = ia_div_up(n, IA_RIG_THREADS);
  int split = ia_div_up(IA_RIG_TARGET_BLOCKS, vblocks);
  if (split > F) split = F;
  if (split > 65535) split = 65535;
  const int fpb = ia_div_up(F, split);
  const dim3 grid(vblocks, ia_div_up(F, fpb));      // grid.y <= split
  const hipStream_t s = (hipStream_t)stream;
  const bool nrm = normals != nullptr;
  if (K <= 4) rig_launch_skin<4>(nrm, grid, s, verts, normals, n, joints, weights, K, bones, F, fpb, out_verts, out_normals);
  else if (K <= 8) rig_launch_skin<8>(nrm, grid, s, verts, normals, n, joints, weights, K, bones, F, fpb, out_verts, out_normals);
  else rig_launch_skin<24>(nrm, grid, s, verts, normals, n, joints, weights, K, bones, F, fpb, out_verts, out_normals);
  IA_LAUNCH_CHECK("k_rig_skin");
  return IA_OK;
}
