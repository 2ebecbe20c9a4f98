// ia_normals.hip -- surface-normal pass behind a rendered frame (no counterpart in the reference, whose geometry figures are
// normal maps of the posed density field): at most one point per pixel,
//   surface point  p = o + (depth / alpha) d                                   (ia_surface_points)
//   canonical candidates of p, sigma AND d sigma / d x_c of every candidate    (ia_snarf_search_compact, ia_field_sigma_grad)
//   arg-max of sigma over the candidates of a point                            (ia_candidate_select)
//   n = -M^{-T} g / |M^{-T} g|, M = linear part of the blended bone transform  (ia_normals_from_gradient)
//   8-bit images of (n + 1) / 2 and of max(0, n . l)                           (ia_pack_normals8)
// The definition is stated in DESIGN.md section 4 and in include/instantavatar_hip_normals.h.  Nothing here synchronises, allocates or reads on the host.
//
// The vector types, the A fragments of the sigma network (frag_value, pack_slab, MFMA), the normalisation of a sample and the
// cell / corner arithmetic of a hash-grid level come from ia_field_dev.h, which ia_field.hip uses too.
#include "ia_common.h"
#include "ia_field_dev.h"
#include "ia_search_dev.h"
#include "../../include/instantavatar_hip_normals.h"

// ---------------------------------------------------------------------------------------------------------------------
// surface points: deterministic compaction in ray order
// ---------------------------------------------------------------------------------------------------------------------
#define IA_SP_THREADS 256

// a pixel has a surface point when alpha >= 0.5 and t = depth / alpha is finite (a NaN alpha or depth gives none)
__device__ __forceinline__ bool surface_hit(const float *__restrict__ depth, const float *__restrict__ alpha, int i, int R, float &t) {
  t = 0.f;
  if (i >= R) return false;
  const float a = alpha[i];
  if (!(a >= 0.5f)) return false;
  t = depth[i] / a;
  return __builtin_fabsf(t) < INFINITY;   // false for NaN too
}

__global__ __launch_bounds__(IA_SP_THREADS) void k_surface_count(const float *__restrict__ depth, const float *__restrict__ alpha,
                                                                 int R, int32_t *__restrict__ block_cnt) {
  __shared__ int s_w[IA_SP_THREADS / 64];
  const int i = blockIdx.x * IA_SP_THREADS + threadIdx.x;
  float t;
  const bool hit = surface_hit(depth, alpha, i, R, t);
  const int c = __popcll(__ballot(hit));
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < IA_SP_THREADS / 64; w++) s += s_w[w];
    block_cnt[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(IA_SP_THREADS) void k_surface_write(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                                 const float *__restrict__ depth, const float *__restrict__ alpha,
                                                                 int R, const int32_t *__restrict__ block_cnt,
                                                                 float *__restrict__ pts, int32_t *__restrict__ ray_idx,
                                                                 int32_t *__restrict__ n_pts) {
  __shared__ int s_part[IA_SP_THREADS / 64];
  __shared__ int s_w[IA_SP_THREADS / 64];
  // points of all blocks in front of this one (integer sums: any order gives the same offset)
  int before = 0;
  for (int b = threadIdx.x; b < (int)blockIdx.x; b += IA_SP_THREADS) before += block_cnt[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
  const int i = blockIdx.x * IA_SP_THREADS + threadIdx.x;
  float t;
  const bool hit = surface_hit(depth, alpha, i, R, t);
  const unsigned long long m = __ballot(hit);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_part[wave] = before; s_w[wave] = __popcll(m); }
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int w = 0; w < IA_SP_THREADS / 64; w++) {
    base += s_part[w];
    if (w < wave) base += s_w[w];
  }
  if (hit) {
    const int k = base + __popcll(m & ((1ull << lane) - 1ull));
    // o + t d spelled as fma, like the marcher
#pragma unroll
    for (int d = 0; d < 3; d++) pts[(size_t)k * 3 + d] = __builtin_fmaf(t, rays_d[(size_t)i * 3 + d], rays_o[(size_t)i * 3 + d]);
    ray_idx[k] = i;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    int tot = 0;
#pragma unroll
    for (int w = 0; w < IA_SP_THREADS / 64; w++) tot += s_part[w] + s_w[w];
    *n_pts = tot;
  }
}

extern "C" size_t ia_surface_points_workspace_bytes(int R) {
  return ia_align((size_t)ia_div_up(R > 0 ? R : 1, IA_SP_THREADS) * sizeof(int32_t));
}

extern "C" int ia_surface_points(const float *rays_o, const float *rays_d, const float *depth, const float *alpha, int R,
                                 float *pts, int32_t *ray_idx, int32_t *n_pts, void *ws, size_t ws_bytes, void *stream) {
  IA_CHECK_ARG(R >= 0, "ia_surface_points: R < 0");
  IA_CHECK_ARG(n_pts, "ia_surface_points: null pointer");
  IA_CHECK_ARG(ws && (R == 0 || (rays_o && rays_d && depth && alpha && pts && ray_idx)), "ia_surface_points: null pointer");
  if (ws_bytes < ia_surface_points_workspace_bytes(R)) return ia_set_error(IA_ERR_WORKSPACE, "ia_surface_points: workspace too small");
  const int blocks = ia_div_up(R > 0 ? R : 1, IA_SP_THREADS);   // (R == 0: one block that writes *n_pts = 0)
  int32_t *block_cnt = (int32_t *)ws;
  hipLaunchKernelGGL(k_surface_count, dim3(blocks), dim3(IA_SP_THREADS), 0, (hipStream_t)stream, depth, alpha, R, block_cnt);
  hipLaunchKernelGGL(k_surface_write, dim3(blocks), dim3(IA_SP_THREADS), 0, (hipStream_t)stream, rays_o, rays_d, depth, alpha, R,
                     block_cnt, pts, ray_idx, n_pts);
  IA_LAUNCH_CHECK("k_surface_write");
  return IA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// sigma and d sigma / d x of the sigma network in one kernel
// ---------------------------------------------------------------------------------------------------------------------
// Forward: ia_field.hip's chain on the shared device functions -- one lane encodes one sample (per level: eight corner
// products in fp32, rounded to half and accumulated in half, in corner order), lanes j and j + 32 exchange half of their
// levels, the two 32-sample column blocks go through the SAME MFMA sequence with the same A fragments (sigma-net layer 1 [64 x 2L], ReLU + rounding to half,
// layer 2 [16 x 64]); sigma = half(out[0]).  Same operands in the same instructions: the same bits.
// Backward (one output channel: a GEMV chain per sample, no MFMA): the C/D layout leaves hidden unit 32 rb + (r & 3) +
// 8 (r >> 2) + 4 h of sample j in register r of accumulator rb of lane (j, h).  Each of the two lanes forms
//   dF[m] = sum over ITS 32 hidden units of  [half(relu(h1_k)) > 0] W2[0][k] W1[k][m]        (fp32, m < 2L)
// with W1 rows read from LDS (all lanes of a half-wave read the same row: broadcast reads, no bank conflicts), the halves
// are added across lane ^ 32, and the lane that encoded the sample contracts dF with the per-level derivative of the
// trilinear interpolation (the corners are gathered a second time for it, see the kernel):
//   d sigma / d x_d = [0 < raw_d < 1] / scale_d  sum_l  (dfeat_l / dxn_d) . dF[2l, 2l + 1]
// -- the quantity ia_hashgrid_bwd's `dx` defines (ia_field.hip, k_hashgrid_bwd), regrouped.  No table gradient, no
// activation record, no atomics.
#define IA_SG_THREADS 256
#define IA_SG_WAVES (IA_SG_THREADS / 64)

// fractional position and the eight corner entries of one level for one sample, in corner order
__device__ __forceinline__ void sg_corners(const uint32_t *__restrict__ tab, float scale, uint32_t res, uint32_t size, bool hashed,
                                           const float xn[3], float w[3], uint32_t raw[8]) {
  uint32_t g[3];
  pos_fract(xn, scale, g, w);
#pragma unroll
  for (int idx = 0; idx < 8; idx++)
    raw[idx] = tab[corner_index(hashed, g[0] + (idx & 1), g[1] + ((idx >> 1) & 1), g[2] + ((idx >> 2) & 1), res, size)];
}

// packed (f0, f1) half2 of one level: the accumulation of ia_field.hip's level_reduce<2>, which defines it, on a flat raw[8]
__device__ __forceinline__ uint32_t sg_level_feat(const float w[3], const uint32_t raw[8]) {
  _Float16 r0 = (_Float16)0.f, r1 = (_Float16)0.f;
#pragma unroll
  for (int idx = 0; idx < 8; idx++) {
    float wt = 1.f;
    wt *= (idx & 1) ? w[0] : 1.f - w[0];
    wt *= (idx & 2) ? w[1] : 1.f - w[1];
    wt *= (idx & 4) ? w[2] : 1.f - w[2];
    union { uint32_t u; half2v h; } c;
    c.u = raw[idx];
    r0 = r0 + (_Float16)(wt * (float)c.h.x);
    r1 = r1 + (_Float16)(wt * (float)c.h.y);
  }
  union { uint32_t u; half2v h; } o;
  o.h.x = r0; o.h.y = r1;
  return o.u;
}

// gx += scale * sum over corners of (d w_corner / d pos) <t_corner, (d0, d1)>: k_hashgrid_bwd's dx term of one level
__device__ __forceinline__ void sg_level_dx(const float w[3], const uint32_t raw[8], float scale, float d0, float d1, float gx[3]) {
  float a[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int idx = 0; idx < 8; idx++) {
    const float wx = (idx & 1) ? w[0] : 1.f - w[0], wy = (idx & 2) ? w[1] : 1.f - w[1], wz = (idx & 4) ? w[2] : 1.f - w[2];
    union { uint32_t u; half2v h; } c;
    c.u = raw[idx];
    const float dot = __builtin_fmaf((float)c.h.y, d1, (float)c.h.x * d0);
    a[0] = __builtin_fmaf((idx & 1) ? wy * wz : -(wy * wz), dot, a[0]);
    a[1] = __builtin_fmaf((idx & 2) ? wx * wz : -(wx * wz), dot, a[1]);
    a[2] = __builtin_fmaf((idx & 4) ? wx * wy : -(wx * wy), dot, a[2]);
  }
#pragma unroll
  for (int d = 0; d < 3; d++) gx[d] = __builtin_fmaf(scale, a[d], gx[d]);
}

// levels are processed in groups of four: the gathers of a group are in flight together, and the barrier keeps the compiler
// from hoisting the next group's loads above this group's arithmetic (which spills: ia_field.hip, encode_all)
#define IA_SG_GROUP 4
#define IA_SG_GROUP_FENCE() do { asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)

template <int L>
__global__ __launch_bounds__(IA_SG_THREADS) void k_sigma_grad(const float *__restrict__ x, int V, const int32_t *__restrict__ n_dev,
                                                              FieldDev F, float *__restrict__ sigma, float *__restrict__ grad) {
  __shared__ __attribute__((aligned(16))) half8 s_frag[8][64];       // 8 KB
  __shared__ __attribute__((aligned(16))) _Float16 s_w1[64 * 2 * L];  // 4 KB (L = 16), row-major [64][2L]
  __shared__ float s_w2[64];                                         // row 0 of layer 2
  if (n_dev) V = min(V, *n_dev);
  const int n_tiles = (V + 63) >> 6;
  if ((int)blockIdx.x * IA_SG_WAVES >= n_tiles) return;   // whole workgroup idle
  if (F.frags) {
    const uint4 *src = reinterpret_cast<const uint4 *>(F.frags);
    uint4 *dst = reinterpret_cast<uint4 *>(&s_frag[0][0]);
    for (int e = threadIdx.x; e < 8 * 64; e += IA_SG_THREADS) dst[e] = src[e];
  } else {
    for (int e = threadIdx.x; e < 8 * 64 * 8; e += IA_SG_THREADS) {
      const int f = e >> 9, l = (e >> 3) & 63, p = e & 7;
      reinterpret_cast<_Float16 *>(&s_frag[f][l])[p] = frag_value<L>(F, f, l & 31, l >> 5, p);
    }
  }
  for (int e = threadIdx.x; e < 64 * 2 * L; e += IA_SG_THREADS) s_w1[e] = ld_h(F.sig_w1, e);
  if (threadIdx.x < 64) s_w2[threadIdx.x] = (float)ld_h(F.sig_w2, threadIdx.x);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int h = lane >> 5, j = lane & 31;
  for (int tile = blockIdx.x * IA_SG_WAVES + wave; tile < n_tiles; tile += gridDim.x * IA_SG_WAVES) {
    const int i = tile * 64 + lane;
    float xn[3] = {0.f, 0.f, 0.f};
    bool inside[3] = {false, false, false};
    if (i < V) {
      normalise(F, x, (size_t)i, xn);
      // d xn / d x = 1 / scale inside the unit cube, 0 where the clamp is active (xn is exactly 0 or 1 there; NaN: 0 as well)
#pragma unroll
      for (int d = 0; d < 3; d++) inside[d] = xn[d] > 0.f && xn[d] < 1.f;
    }
    uint32_t feat[L];
#pragma unroll
    for (int l0 = 0; l0 < L; l0 += IA_SG_GROUP) {
      float w[IA_SG_GROUP][3];
      uint32_t raw[IA_SG_GROUP][8];
#pragma unroll
      for (int k = 0; k < IA_SG_GROUP; k++)
        sg_corners(F.table + F.lv.offset[l0 + k], F.lv.scale[l0 + k], F.lv.res[l0 + k], F.lv.size[l0 + k], F.lv.hashed[l0 + k] != 0, xn,
                   w[k], raw[k]);
#pragma unroll
      for (int k = 0; k < IA_SG_GROUP; k++) feat[l0 + k] = sg_level_feat(w[k], raw[k]);
      IA_SG_GROUP_FENCE();
    }
    // lane j gives its upper-half levels to lane j + 32 and receives that lane's lower-half levels
#pragma unroll
    for (int q = 0; q < L / 2; q++) {
      auto r = __builtin_amdgcn_permlane32_swap(feat[q], feat[q + L / 2], false, false);
      feat[q] = r[0];
      feat[q + L / 2] = r[1];
    }
    float dF[2 * L];
#pragma unroll
    for (int m = 0; m < 2 * L; m++) dF[m] = 0.f;
#pragma unroll
    for (int cb = 0; cb < 2; cb++) {
      floatx16 a1[2], a2;
#pragma unroll
      for (int rb = 0; rb < 2; rb++) {
        a1[rb] = (floatx16){0.f};
#pragma unroll
        for (int s = 0; s < L / 8; s++) {
          union { uint32_t u[4]; half8 v; } b;
#pragma unroll
          for (int q = 0; q < 4; q++) b.u[q] = feat[cb * (L / 2) + 4 * s + q];
          a1[rb] = MFMA(s_frag[rb * 2 + s][lane], b.v, a1[rb]);
        }
      }
      a2 = (floatx16){0.f};
#pragma unroll
      for (int s = 0; s < 4; s++)
        a2 = MFMA(s_frag[4 + s][lane], (s & 1) ? pack_slab<true>(a1[s >> 1], 1) : pack_slab<true>(a1[s >> 1], 0), a2);
      const int o = tile * 64 + cb * 32 + j;
      if (h == 0 && o < V) sigma[o] = (float)(_Float16)a2[0];   // row 0 lives in lanes h == 0
      // ---- backward through this lane's 32 hidden units ----
      float acc[2 * L];
#pragma unroll
      for (int m = 0; m < 2 * L; m++) acc[m] = 0.f;
      uint32_t on = 0u;   // bit 16 rb + r: the forward's half-rounded hidden unit is active
#pragma unroll
      for (int rb = 0; rb < 2; rb++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const float v = a1[rb][r];
          on |= ((float)(_Float16)(v < 0.f ? 0.f : v) > 0.f) ? (1u << (16 * rb + r)) : 0u;
        }
      // (a rolled loop over the lane's 32 units, the mask in a register: unrolled, the weight rows of all 32 are hoisted and spill)
#pragma unroll 2
      for (int t = 0; t < 32; t++) {
        const int k = 32 * (t >> 4) + cd_row(t & 15, h);
        const float dh = ((on >> t) & 1u) ? s_w2[k] : 0.f;
        const half8 *row = reinterpret_cast<const half8 *>(s_w1 + k * 2 * L);
#pragma unroll
        for (int q = 0; q < 2 * L / 8; q++) {
          const half8 wv = row[q];
#pragma unroll
          for (int p = 0; p < 8; p++) acc[8 * q + p] = __builtin_fmaf(dh, (float)wv[p], acc[8 * q + p]);
        }
      }
#pragma unroll
      for (int m = 0; m < 2 * L; m++) {
        const float tot = acc[m] + __shfl_xor(acc[m], 32, 64);
        if (cb == h) dF[m] = tot;   // the lane that encoded sample 32 cb + j
      }
    }
    // contraction with the derivative of the trilinear interpolation: the corners are gathered a second time (cache hits)
    // instead of keeping 6 floats per level alive across the MLP -- that version spilled
    float gx[3] = {0.f, 0.f, 0.f};
    // (opaque copy of the position: otherwise the compiler keeps the 8 L corner indices of the encoding alive across the MLP)
    asm volatile("" : "+v"(xn[0]), "+v"(xn[1]), "+v"(xn[2]));
#pragma unroll
    for (int l0 = 0; l0 < L; l0 += IA_SG_GROUP) {
      float w[IA_SG_GROUP][3];
      uint32_t raw[IA_SG_GROUP][8];
#pragma unroll
      for (int k = 0; k < IA_SG_GROUP; k++)
        sg_corners(F.table + F.lv.offset[l0 + k], F.lv.scale[l0 + k], F.lv.res[l0 + k], F.lv.size[l0 + k], F.lv.hashed[l0 + k] != 0, xn,
                   w[k], raw[k]);
#pragma unroll
      for (int k = 0; k < IA_SG_GROUP; k++) sg_level_dx(w[k], raw[k], F.lv.scale[l0 + k], dF[2 * (l0 + k)], dF[2 * (l0 + k) + 1], gx);
      IA_SG_GROUP_FENCE();
    }
    if (i < V) {
#pragma unroll
      for (int d = 0; d < 3; d++) grad[(size_t)i * 3 + d] = inside[d] ? gx[d] / F.scale[d] : 0.f;
    }
  }
}

extern "C" int ia_field_sigma_grad(const float *x, int V, const int32_t *n_dev, const ia_field *field, float *sigma, float *grad,
                                   void *stream) {
  IA_CHECK_ARG(V >= 0, "ia_field_sigma_grad: V < 0");
  if (V == 0) return IA_OK;
  IA_CHECK_ARG(x && sigma && grad, "ia_field_sigma_grad: null pointer");
  FieldDev F;
  const int rc = ia_make_field_dev(field, &F);
  IA_CHECK_ARG(rc == 0, "ia_field_sigma_grad: bad field descriptor (%d)", rc);
  const int tiles = ia_div_up(V, 64);
  int blocks = ia_div_up(tiles, IA_SG_WAVES);
  if (blocks > 2048) blocks = 2048;   // workgroups loop over their tiles
  if (F.lv.n_levels == 16)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sigma_grad<16>), dim3(blocks), dim3(IA_SG_THREADS), 0, (hipStream_t)stream, x, V, n_dev, F, sigma, grad);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sigma_grad<8>), dim3(blocks), dim3(IA_SG_THREADS), 0, (hipStream_t)stream, x, V, n_dev, F, sigma, grad);
  IA_LAUNCH_CHECK("k_sigma_grad");
  return IA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// arg-max of sigma over a point's valid candidates (first maximum wins; a non-finite sigma counts as 0, as deform_test's
// nan_to_num makes it): root and gradient of the winner, zeros for a point without a candidate
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_candidate_select(const float *__restrict__ cand_sigma, const float *__restrict__ cand_xc,
                                                          const float *__restrict__ cand_grad, int cand_cap,
                                                          const int32_t *__restrict__ pt_off, const uint8_t *__restrict__ pt_cnt, int P,
                                                          const int32_t *__restrict__ n_pts_dev, float *__restrict__ root,
                                                          float *__restrict__ grad, int32_t *__restrict__ arg) {
  if (n_pts_dev) P = min(P, *n_pts_dev);
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const int off = pt_off[p], cnt = pt_cnt[p];
  float best = -INFINITY;
  int bi = -1;
  for (int c = 0; c < cnt && off + c < cand_cap; c++) {
    float s = cand_sigma[off + c];
    if (!(__builtin_fabsf(s) < INFINITY)) s = 0.f;
    if (s > best) { best = s; bi = off + c; }
  }
#pragma unroll
  for (int d = 0; d < 3; d++) {
    root[(size_t)p * 3 + d] = bi >= 0 ? cand_xc[(size_t)bi * 3 + d] : 0.f;
    grad[(size_t)p * 3 + d] = bi >= 0 ? cand_grad[(size_t)bi * 3 + d] : 0.f;
  }
  if (arg) arg[p] = bi;
}

extern "C" int ia_candidate_select(const float *cand_sigma, const float *cand_xc, const float *cand_grad, int cand_cap,
                                   const int32_t *pt_off, const uint8_t *pt_cnt, int P, const int32_t *n_pts_dev, float *root,
                                   float *grad, int32_t *arg, void *stream) {
  IA_CHECK_ARG(P >= 0 && cand_cap >= 0, "ia_candidate_select: negative size");
  if (P == 0) return IA_OK;
  IA_CHECK_ARG(cand_sigma && cand_xc && cand_grad && pt_off && pt_cnt && root && grad, "ia_candidate_select: null pointer");
  hipLaunchKernelGGL(k_candidate_select, dim3(ia_div_up(P, 256)), dim3(256), 0, (hipStream_t)stream, cand_sigma, cand_xc, cand_grad,
                     cand_cap, pt_off, pt_cnt, P, n_pts_dev, root, grad, arg);
  IA_LAUNCH_CHECK("k_candidate_select");
  return IA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// normals from gradients
// ---------------------------------------------------------------------------------------------------------------------
// One lane = one point.  M = linear part of the trilinearly interpolated transform grid at the root (the search's fetch:
// 8 corner records of 48 B, corners outside the grid with weight 0), v = cof(M) g (= det(M) M^{-T} g, rows of cof(M) are
// the cross products of the rows of M), n = -sign(det) v, rotated by the transpose of w2s' rotation and normalised.
// Zero (the map's fill value is left in place) when g = 0, det(M) = 0 or anything is not finite.
__global__ __launch_bounds__(256) void k_normals(const float *__restrict__ root, const float *__restrict__ grad,
                                                 const int32_t *__restrict__ ray_idx, int n, const int32_t *__restrict__ n_dev,
                                                 const float *__restrict__ voxel_J, SnarfGridDev G, const float *__restrict__ w2s, int R,
                                                 float *__restrict__ normals) {
  if (n_dev) n = min(n, *n_dev);
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int ray = ray_idx[p];
  if ((uint32_t)ray >= (uint32_t)R) return;
  const float x0 = root[(size_t)p * 3], x1 = root[(size_t)p * 3 + 1], x2 = root[(size_t)p * 3 + 2];
  const float g0 = grad[(size_t)p * 3], g1 = grad[(size_t)p * 3 + 1], g2 = grad[(size_t)p * 3 + 2];
  FetchPlan fp;
  fetch_plan(G, G.scl[0] * (x0 + G.off[0]), G.scl[1] * (x1 + G.off[1]), G.scl[2] * (x2 + G.off[2]), true, fp);
  if (fp.load == 0) return;   // every corner outside the grid: M = 0
  float M[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const char *vJb = reinterpret_cast<const char *>(voxel_J);
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const float4 *rec = reinterpret_cast<const float4 *>(vJb + (size_t)fp.off[c]);
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const float4 v = rec[r];
      M[3 * r] = __builtin_fmaf(v.x, fp.w[c], M[3 * r]);
      M[3 * r + 1] = __builtin_fmaf(v.y, fp.w[c], M[3 * r + 1]);
      M[3 * r + 2] = __builtin_fmaf(v.z, fp.w[c], M[3 * r + 2]);
    }
  }
  // cofactor rows
  const float c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
  const float c10 = M[7] * M[2] - M[8] * M[1], c11 = M[8] * M[0] - M[6] * M[2], c12 = M[6] * M[1] - M[7] * M[0];
  const float c20 = M[1] * M[5] - M[2] * M[4], c21 = M[2] * M[3] - M[0] * M[5], c22 = M[0] * M[4] - M[1] * M[3];
  const float det = IA_DOT3(M[0], c00, M[1], c01, M[2], c02);
  if (!(__builtin_fabsf(det) < INFINITY) || det == 0.f) return;
  // scale g first: the products below then neither overflow nor underflow for any finite gradient
  const float gm = fmaxf(fmaxf(__builtin_fabsf(g0), __builtin_fabsf(g1)), __builtin_fabsf(g2));
  if (!(gm < INFINITY) || gm == 0.f) return;
  const float sg = (det > 0.f ? -1.f : 1.f) / gm;
  const float h0 = g0 * sg, h1 = g1 * sg, h2 = g2 * sg;
  const float v0 = IA_DOT3(c00, h0, c01, h1, c02, h2), v1 = IA_DOT3(c10, h0, c11, h1, c12, h2), v2 = IA_DOT3(c20, h0, c21, h1, c22, h2);
  // camera frame: w2s maps camera -> SMPL root (x_s = R x_w + t), so n_w = R^T n_s
  float u[3];
#pragma unroll
  for (int d = 0; d < 3; d++) u[d] = IA_DOT3(w2s[d], v0, w2s[4 + d], v1, w2s[8 + d], v2);
  const float um = fmaxf(fmaxf(__builtin_fabsf(u[0]), __builtin_fabsf(u[1])), __builtin_fabsf(u[2]));
  if (!(um < INFINITY) || um == 0.f) return;
  u[0] /= um; u[1] /= um; u[2] /= um;
  const float len = sqrtf(IA_DOT3(u[0], u[0], u[1], u[1], u[2], u[2]));
#pragma unroll
  for (int d = 0; d < 3; d++) normals[(size_t)ray * 3 + d] = u[d] / len;
}

extern "C" int ia_normals_from_gradient(const float *root, const float *grad, const int32_t *ray_idx, int n, const int32_t *n_dev,
                                        const float *voxel_J, const ia_snarf_grid *grid, const float *w2s, int R, float *normals,
                                        void *stream) {
  IA_CHECK_ARG(n >= 0 && R >= 0, "ia_normals_from_gradient: negative size");
  if (R == 0) return IA_OK;
  IA_CHECK_ARG(normals, "ia_normals_from_gradient: null pointer");
  // the map is zero-filled by a kernel, not by a memset node (NOTES.md: replayed graphs); 12 R bytes, 16-byte stores
  IA_CHECK_ARG((reinterpret_cast<uintptr_t>(normals) & 15) == 0, "ia_normals_from_gradient: the map must be 16-byte aligned");
  ia_zero_fill(normals, (size_t)R * 12, (hipStream_t)stream);
  if (n > 0) {
    IA_CHECK_ARG(root && grad && ray_idx && voxel_J && grid && w2s, "ia_normals_from_gradient: null pointer");
    IA_CHECK_ARG(grid->D > 0 && grid->H > 0 && grid->W > 0 && (long)grid->D * grid->H * grid->W * 48 < (1l << 32),
                 "ia_normals_from_gradient: bad grid");
    hipLaunchKernelGGL(k_normals, dim3(ia_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, root, grad, ray_idx, n, n_dev, voxel_J,
                       ia_make_grid_dev(grid), w2s, R, normals);
  }
  IA_LAUNCH_CHECK("k_normals");
  return IA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the two 8-bit images of a normal map, one launch: normal_rgba = ((n + 1) / 2, covered) and shaded_rgba = (s, s, s, covered),
// s = max(0, n . l), l = `light` (device float[3], normalised here) or, when NULL, the direction towards the camera of the
// pixel's own ray (-rays_d); covered = 255 where the pixel has a normal, 0 (and all channels 0) elsewhere.  Quantised like
// ia_pack_rgba8: (uint8)(clamp(v, 0, 1) * 255).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pack_normals8(const float *__restrict__ normals, const float *__restrict__ rays_d,
                                                       const float *__restrict__ light, int R, uint32_t *__restrict__ normal_rgba,
                                                       uint32_t *__restrict__ shaded_rgba) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R) return;
  const float n0 = normals[3 * (size_t)i], n1 = normals[3 * (size_t)i + 1], n2 = normals[3 * (size_t)i + 2];
  if (n0 == 0.f && n1 == 0.f && n2 == 0.f) {
    normal_rgba[i] = 0u;
    shaded_rgba[i] = 0u;
    return;
  }
  auto q = [](float v) -> uint32_t { return (uint32_t)(fminf(fmaxf(v, 0.f), 1.f) * 255.f); };
  normal_rgba[i] = q((n0 + 1.f) * 0.5f) | (q((n1 + 1.f) * 0.5f) << 8) | (q((n2 + 1.f) * 0.5f) << 16) | (255u << 24);
  float l0, l1, l2;
  if (light) { l0 = light[0]; l1 = light[1]; l2 = light[2]; }
  else { l0 = -rays_d[3 * (size_t)i]; l1 = -rays_d[3 * (size_t)i + 1]; l2 = -rays_d[3 * (size_t)i + 2]; }
  const float ll = sqrtf(IA_DOT3(l0, l0, l1, l1, l2, l2));
  const float s = ll > 0.f ? IA_DOT3(n0, l0, n1, l1, n2, l2) / ll : 0.f;
  const uint32_t qs = q(s);   // (NaN -> fmaxf gives 0)
  shaded_rgba[i] = qs | (qs << 8) | (qs << 16) | (255u << 24);
}

extern "C" int ia_pack_normals8(const float *normals, const float *rays_d, const float *light, int R, uint8_t *normal_rgba,
                                uint8_t *shaded_rgba, void *stream) {
  IA_CHECK_ARG(R >= 0, "ia_pack_normals8: R < 0");
  if (R == 0) return IA_OK;
  IA_CHECK_ARG(normals && normal_rgba && shaded_rgba && (light || rays_d), "ia_pack_normals8: null pointer");
  IA_CHECK_ARG(((reinterpret_cast<uintptr_t>(normal_rgba) | reinterpret_cast<uintptr_t>(shaded_rgba)) & 3) == 0,
               "ia_pack_normals8: the images must be 4-byte aligned");
  hipLaunchKernelGGL(k_pack_normals8, dim3(ia_div_up(R, 256)), dim3(256), 0, (hipStream_t)stream, normals, rays_d, light, R,
                     reinterpret_cast<uint32_t *>(normal_rgba), reinterpret_cast<uint32_t *>(shaded_rgba));
  IA_LAUNCH_CHECK("k_pack_normals8");
  return IA_OK;
}
