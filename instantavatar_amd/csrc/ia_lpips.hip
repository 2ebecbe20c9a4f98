// ia_lpips.hip -- the patch terms of the fit stage's loss (include/instantavatar_hip_lpips.h; definition in DESIGN.md section 4, "patch
// loss"): the 3 x 3 convolution of the frozen VGG-16 trunk and of its adjoint as an implicit GEMM on the exact fp32 MFMA, the 2 x 2
// max-pool and its gradient, the LPIPS input preparation and head with their gradients, and the depth regulariser.
//
// ia_conv3x3.  D[co][pixel] = sum_k Wp[k][co] X[k][pixel], k = 9 ci + tap: the weights are the MFMA's A operand, the gathered input
// (im2col, never materialised) its B operand, so that the 16 lanes of a result column group hold 16 consecutive pixels of one channel
// and the NCHW store is contiguous.  A workgroup of four waves owns 64 channels x 64 pixels of one K chunk (288 rows = 32 input channels);
// each wave 32 x 32 of it as 2 x 2 tiles of v_mfma_f32_16x16x4_f32, i.e. four independent accumulators (the instruction's dependent
// latency is 40 cycles at a 32-cycle issue).  Operand tiles of 32 k-rows go through LDS, rows padded from 64 to 80 floats: the
// fragment read of lane l is row (l >> 4), column (l & 15), and with 80-float rows lanes l and l + 16 fall on different banks.  The next
// tile's global loads are issued before the current tile's MFMAs.  The MFMA is a k-ordered fma chain, so an output element's bits depend
// on its own row of X and column of Wp only -- not on the tile it falls into, nor on the batch.
#include "ia_common.h"
#include "../../include/instantavatar_hip_lpips.h"

typedef float cv_f32x4 __attribute__((ext_vector_type(4)));

#define CV_TILE 64        // output channels and pixels per workgroup
#define CV_KB 32          // k rows per LDS tile
#define CV_LD 80          // LDS row stride in floats
#define CV_CHUNK_K (9 * IA_CONV3X3_CHUNK_CHANNELS)
#define CV_TILES_PER_CHUNK (CV_CHUNK_K / CV_KB)

static inline int cv_chunks(int Cin) { return (Cin + IA_CONV3X3_CHUNK_CHANNELS - 1) / IA_CONV3X3_CHUNK_CHANNELS; }
static inline int cv_cpad(int Cout) { return (Cout + CV_TILE - 1) / CV_TILE * CV_TILE; }
static inline bool cv_channels_ok(int Cin, int Cout) {
  return Cin >= 1 && Cout >= 1 && Cin <= IA_CONV3X3_MAX_CHANNELS && Cout <= IA_CONV3X3_MAX_CHANNELS;
}
static inline bool cv_shape_ok(int N, int Cin, int Cout, int H, int W) {
  if (!cv_channels_ok(Cin, Cout) || N < 1 || H < 1 || W < 1) return false;
  const long long lim = 1LL << 31, c = Cin > Cout ? Cin : Cout;
  long long v = (long long)N * H;
  if (v >= lim) return false;
  v *= W;
  if (v >= lim) return false;
  return v * c < lim;
}

// ---- weight image ----------------------------------------------------------------------------------------------------------------
__global__ void k_conv_pack(const float *__restrict__ w, int Cin_w, int Cin, int Cout, int Cp, int total, int tf, float *__restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int k = idx / Cp, co = idx - k * Cp, ci = k / 9, tap = k - 9 * ci;
  float v = 0.f;
  if (ci < Cin && co < Cout)
    v = tf ? w[((size_t)ci * Cin_w + co) * 9 + (8 - tap)] : w[((size_t)co * Cin_w + ci) * 9 + tap];
  out[idx] = v;
}

extern "C" size_t ia_conv3x3_packed_bytes(int Cin, int Cout) {
  if (!cv_channels_ok(Cin, Cout)) return 0;
  return (size_t)cv_chunks(Cin) * CV_CHUNK_K * cv_cpad(Cout) * sizeof(float);
}

extern "C" int ia_conv3x3_pack(const float *w, int Cout_w, int Cin_w, int transpose_flip, float *packed, size_t packed_bytes, void *stream) {
  IA_CHECK_ARG(cv_channels_ok(Cin_w, Cout_w), "ia_conv3x3_pack: weights [%d,%d,3,3]: 1 .. %d channels", Cout_w, Cin_w, IA_CONV3X3_MAX_CHANNELS);
  IA_CHECK_ARG(w && packed, "ia_conv3x3_pack: w and packed are required");
  const int Cin = transpose_flip ? Cout_w : Cin_w, Cout = transpose_flip ? Cin_w : Cout_w;
  const size_t need = ia_conv3x3_packed_bytes(Cin, Cout);
  IA_CHECK_ARG(packed_bytes >= need, "ia_conv3x3_pack: packed of %zu bytes, %zu needed (ia_conv3x3_packed_bytes)", packed_bytes, need);
  IA_CHECK_ARG(((uintptr_t)packed & 15) == 0, "ia_conv3x3_pack: packed must be 16-byte aligned");
  const int Cp = cv_cpad(Cout), total = (int)(need / sizeof(float));
  hipLaunchKernelGGL(k_conv_pack, dim3(ia_div_up(total, 256)), dim3(256), 0, (hipStream_t)stream, w, Cin_w, Cin, Cout, Cp, total,
                     transpose_flip ? 1 : 0, packed);
  IA_LAUNCH_CHECK("k_conv_pack");
  return IA_OK;
}

// ---- convolution -----------------------------------------------------------------------------------------------------------------
struct ConvArgs {
  const float *x, *gate, *wp, *bias;
  float *y, *part;
  int N, Cin, Cout, Cp, H, W, HW, M, relu, S;
  size_t total;   // N Cout H W
};

__device__ __forceinline__ void cv_load(const ConvArgs &A, int kb, int co0, int t, bool mval, int n, int py, int px, cv_f32x4 &Ra0, cv_f32x4 &Ra1,
                                        float (&Rb)[8]) {
  const int ar = t >> 4, ac = (t & 15) * 4, bq = t >> 6;
  Ra0 = *(const cv_f32x4 *)(A.wp + (size_t)(kb + ar) * A.Cp + co0 + ac);
  Ra1 = *(const cv_f32x4 *)(A.wp + (size_t)(kb + ar + 16) * A.Cp + co0 + ac);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int k = kb + bq + 4 * j, ci = k / 9, tap = k - 9 * ci, dy = tap / 3, dx = tap - 3 * dy;
    const int yy = py + dy - 1, xx = px + dx - 1;
    const bool ok = mval && ci < A.Cin && (unsigned)yy < (unsigned)A.H && (unsigned)xx < (unsigned)A.W;
    float v = 0.f;
    if (ok) {
      const size_t idx = ((size_t)(n * A.Cin + ci) * A.H + yy) * A.W + xx;
      v = A.x[idx];
      if (A.gate) v = v * (A.gate[idx] > 0.f ? 1.f : 0.f);
    }
    Rb[j] = v;
  }
}

__global__ __launch_bounds__(256) void k_conv3x3(ConvArgs A) {
  __shared__ __attribute__((aligned(16))) float lds[2 * CV_KB * CV_LD];
  float *As = lds, *Bs = lds + CV_KB * CV_LD;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.x * CV_TILE, co0 = blockIdx.y * CV_TILE, chunk = blockIdx.z;
  // gather role: pixel t & 63 of the tile, k rows (t >> 6) + 4 j
  const int m = m0 + (t & 63);
  const bool mval = m < A.M;
  int n = 0, py = 0, px = 0;
  if (mval) {
    n = m / A.HW;
    const int r = m - n * A.HW;
    py = r / A.W;
    px = r - py * A.W;
  }
  const int wm = wave >> 1, wp = wave & 1, lr = lane & 15, lk = lane >> 4;
  cv_f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = cv_f32x4{0.f, 0.f, 0.f, 0.f};
  cv_f32x4 Ra0, Ra1;
  float Rb[8];
  const int kc0 = chunk * CV_CHUNK_K;
  cv_load(A, kc0, co0, t, mval, n, py, px, Ra0, Ra1, Rb);
  for (int tile = 0; tile < CV_TILES_PER_CHUNK; tile++) {
    {
      const int ar = t >> 4, ac = (t & 15) * 4, bq = t >> 6, bp = t & 63;
      *(cv_f32x4 *)(As + ar * CV_LD + ac) = Ra0;
      *(cv_f32x4 *)(As + (ar + 16) * CV_LD + ac) = Ra1;
#pragma unroll
      for (int j = 0; j < 8; j++) Bs[(bq + 4 * j) * CV_LD + bp] = Rb[j];
    }
    __syncthreads();
    if (tile + 1 < CV_TILES_PER_CHUNK) cv_load(A, kc0 + (tile + 1) * CV_KB, co0, t, mval, n, py, px, Ra0, Ra1, Rb);
#pragma unroll
    for (int ks = 0; ks < CV_KB / 4; ks++) {
      const int k = ks * 4 + lk;
      const float a0 = As[k * CV_LD + wm * 32 + lr], a1 = As[k * CV_LD + wm * 32 + 16 + lr];
      const float b0 = Bs[k * CV_LD + wp * 32 + lr], b1 = Bs[k * CV_LD + wp * 32 + 16 + lr];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
  // D: column (pixel) = lane & 15, row (channel) = 4 (lane >> 4) + register
  float *dst = A.S > 1 ? A.part + (size_t)chunk * A.total : A.y;
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int mo = m0 + wp * 32 + j * 16 + lr;
    if (mo >= A.M) continue;
    const int no = mo / A.HW, ro = mo - no * A.HW;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int co = co0 + wm * 32 + i * 16 + lk * 4 + r;
        if (co >= A.Cout) continue;
        float v = acc[i][j][r];
        if (A.S == 1) {
          if (A.bias) v = v + A.bias[co];
          if (A.relu) v = v > 0.f ? v : 0.f;
        }
        dst[((size_t)no * A.Cout + co) * A.HW + ro] = v;
      }
  }
}

// chunk sums in ascending order, then the bias
__global__ void k_conv_reduce(const float *__restrict__ part, const float *__restrict__ bias, int S, size_t total, int Cout, int HW, int relu,
                              float *__restrict__ y) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  float s = part[idx];
  for (int c = 1; c < S; c++) s = s + part[(size_t)c * total + idx];
  if (bias) s = s + bias[(idx / HW) % Cout];
  if (relu) s = s > 0.f ? s : 0.f;
  y[idx] = s;
}

extern "C" size_t ia_conv3x3_workspace_bytes(int N, int Cin, int Cout, int H, int W) {
  if (!cv_shape_ok(N, Cin, Cout, H, W)) return 0;
  const int S = cv_chunks(Cin);
  return S > 1 ? ia_align((size_t)S * N * Cout * H * W * sizeof(float)) : 256;
}

extern "C" int ia_conv3x3(const float *x, const float *gate, const float *packed, const float *bias, int N, int Cin, int Cout, int H, int W,
                          int relu, float *y, void *ws, size_t ws_bytes, void *stream) {
  IA_CHECK_ARG(cv_shape_ok(N, Cin, Cout, H, W),
               "ia_conv3x3: N %d, Cin %d, Cout %d, H %d, W %d: 1 .. %d channels, N, H, W >= 1 and N H W max(Cin, Cout) < 2^31", N, Cin, Cout, H,
               W, IA_CONV3X3_MAX_CHANNELS);
  IA_CHECK_ARG(x && packed && y, "ia_conv3x3: x, packed and y are required");
  IA_CHECK_ARG(((uintptr_t)packed & 15) == 0, "ia_conv3x3: packed must be 16-byte aligned");
  const int S = cv_chunks(Cin);
  const size_t need = ia_conv3x3_workspace_bytes(N, Cin, Cout, H, W);
  IA_CHECK_ARG(S == 1 || (ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0),
               "ia_conv3x3: workspace of %zu bytes, %zu needed, 16-byte aligned (ia_conv3x3_workspace_bytes)", ws_bytes, need);
  ConvArgs A;
  A.x = x; A.gate = gate; A.wp = packed; A.bias = bias; A.y = y; A.part = (float *)ws;
  A.N = N; A.Cin = Cin; A.Cout = Cout; A.Cp = cv_cpad(Cout); A.H = H; A.W = W; A.HW = H * W; A.M = N * H * W; A.relu = relu ? 1 : 0; A.S = S;
  A.total = (size_t)N * Cout * H * W;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_conv3x3, dim3(ia_div_up(A.M, CV_TILE), A.Cp / CV_TILE, S), dim3(256), 0, s, A);
  IA_LAUNCH_CHECK("k_conv3x3");
  if (S > 1) {
    hipLaunchKernelGGL(k_conv_reduce, dim3(ia_div_up((long)A.total, 256)), dim3(256), 0, s, (const float *)A.part, bias, S, A.total, Cout,
                       A.HW, A.relu, y);
    IA_LAUNCH_CHECK("k_conv_reduce");
  }
  return IA_OK;
}

// ---- 2 x 2 max-pool ----------------------------------------------------------------------------------------------------------------
// the first maximum of the window in row-major order; a NaN wins (torch: `val > max || isnan(val)`)
__device__ __forceinline__ int pool_argmax(const float *__restrict__ p, int W, float &best) {
  int arg = 0;
  best = p[0];
  const float v1 = p[1], v2 = p[W], v3 = p[W + 1];
  if (v1 > best || v1 != v1) { best = v1; arg = 1; }
  if (v2 > best || v2 != v2) { best = v2; arg = 2; }
  if (v3 > best || v3 != v3) { best = v3; arg = 3; }
  return arg;
}

__global__ void k_maxpool(const float *__restrict__ x, int H, int W, int OH, int OW, size_t total, float *__restrict__ y) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const size_t nc = idx / ((size_t)OH * OW);
  const int r = (int)(idx - nc * OH * OW), oy = r / OW, ox = r - oy * OW;
  float best;
  pool_argmax(x + (nc * H + 2 * oy) * W + 2 * ox, W, best);
  y[idx] = best;
}

__global__ void k_maxpool_bwd(const float *__restrict__ x, const float *__restrict__ dy, int H, int W, int OH, int OW, size_t total,
                              float *__restrict__ dx) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const size_t nc = idx / ((size_t)H * W);
  const int r = (int)(idx - nc * H * W), yy = r / W, xx = r - yy * W, oy = yy >> 1, ox = xx >> 1;
  float g = 0.f;
  if (oy < OH && ox < OW) {
    float best;
    const int arg = pool_argmax(x + (nc * H + 2 * oy) * W + 2 * ox, W, best);
    if (arg == (yy & 1) * 2 + (xx & 1)) g = dy[(nc * OH + oy) * OW + ox];
  }
  dx[idx] = g;
}

static inline bool pool_shape_ok(int NC, int H, int W) {
  return NC >= 1 && H >= 2 && W >= 2 && (long long)NC * H * W < (1LL << 31);
}

extern "C" int ia_maxpool2x2(const float *x, int NC, int H, int W, float *y, void *stream) {
  IA_CHECK_ARG(pool_shape_ok(NC, H, W), "ia_maxpool2x2: NC %d, H %d, W %d: NC >= 1, H, W >= 2, NC H W < 2^31", NC, H, W);
  IA_CHECK_ARG(x && y, "ia_maxpool2x2: x and y are required");
  const size_t total = (size_t)NC * (H / 2) * (W / 2);
  hipLaunchKernelGGL(k_maxpool, dim3(ia_div_up((long)total, 256)), dim3(256), 0, (hipStream_t)stream, x, H, W, H / 2, W / 2, total, y);
  IA_LAUNCH_CHECK("k_maxpool");
  return IA_OK;
}

extern "C" int ia_maxpool2x2_bwd(const float *x, const float *dy, int NC, int H, int W, float *dx, void *stream) {
  IA_CHECK_ARG(pool_shape_ok(NC, H, W), "ia_maxpool2x2_bwd: NC %d, H %d, W %d: NC >= 1, H, W >= 2, NC H W < 2^31", NC, H, W);
  IA_CHECK_ARG(x && dy && dx, "ia_maxpool2x2_bwd: x, dy and dx are required");
  const size_t total = (size_t)NC * H * W;
  hipLaunchKernelGGL(k_maxpool_bwd, dim3(ia_div_up((long)total, 256)), dim3(256), 0, (hipStream_t)stream, x, dy, H, W, H / 2, W / 2, total, dx);
  IA_LAUNCH_CHECK("k_maxpool_bwd");
  return IA_OK;
}

// ---- LPIPS input ----------------------------------------------------------------------------------------------------------------------
__global__ void k_lpips_prepare(const float *__restrict__ pred, const float *__restrict__ target, const float *__restrict__ shift,
                                const float *__restrict__ scale, int n, int PQ, size_t total, float *__restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int pq = (int)(idx % PQ), c = (int)((idx / PQ) % 3), i = (int)(idx / ((size_t)3 * PQ));
  float v;
  if (i < n) {
    v = pred[((size_t)i * PQ + pq) * 3 + (2 - c)];
    v = v > 1.f ? 1.f : v;
  } else {
    v = target[((size_t)(i - n) * PQ + pq) * 3 + (2 - c)];
  }
  v = 2.f * v;
  v = v - 1.f;
  v = v - shift[c];
  out[idx] = v / scale[c];
}

__global__ void k_lpips_prepare_bwd(const float *__restrict__ pred, const float *__restrict__ g, const float *__restrict__ scale, int PQ,
                                    size_t total, float *__restrict__ d_pred) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int ch = (int)(idx % 3), c = 2 - ch, pq = (int)((idx / 3) % PQ);
  const size_t i = idx / ((size_t)3 * PQ);
  float d = 0.f;
  if (pred[idx] <= 1.f) {
    d = g[(i * 3 + c) * PQ + pq] / scale[c];
    d = d * 2.f;
  }
  d_pred[idx] = d;
}

static inline bool prep_shape_ok(int n, int P, int Q) {
  return n >= 1 && P >= 1 && Q >= 1 && (long long)P * Q < (1LL << 31) / 6 && (long long)n * P * Q < (1LL << 31) / 6;
}

extern "C" int ia_lpips_prepare(const float *pred, const float *target, const float *shift, const float *scale, int n, int P, int Q,
                                float *out, void *stream) {
  IA_CHECK_ARG(prep_shape_ok(n, P, Q), "ia_lpips_prepare: n %d, P %d, Q %d: all >= 1, 6 n P Q < 2^31", n, P, Q);
  IA_CHECK_ARG(pred && target && shift && scale && out, "ia_lpips_prepare: pred, target, shift, scale and out are required");
  const size_t total = (size_t)2 * n * 3 * P * Q;
  hipLaunchKernelGGL(k_lpips_prepare, dim3(ia_div_up((long)total, 256)), dim3(256), 0, (hipStream_t)stream, pred, target, shift, scale, n,
                     P * Q, total, out);
  IA_LAUNCH_CHECK("k_lpips_prepare");
  return IA_OK;
}

extern "C" int ia_lpips_prepare_bwd(const float *pred, const float *g, const float *scale, int n, int P, int Q, float *d_pred, void *stream) {
  IA_CHECK_ARG(prep_shape_ok(n, P, Q), "ia_lpips_prepare_bwd: n %d, P %d, Q %d: all >= 1, 6 n P Q < 2^31", n, P, Q);
  IA_CHECK_ARG(pred && g && scale && d_pred, "ia_lpips_prepare_bwd: pred, g, scale and d_pred are required");
  const size_t total = (size_t)n * 3 * P * Q;
  hipLaunchKernelGGL(k_lpips_prepare_bwd, dim3(ia_div_up((long)total, 256)), dim3(256), 0, (hipStream_t)stream, pred, g, scale, P * Q, total,
                     d_pred);
  IA_LAUNCH_CHECK("k_lpips_prepare_bwd");
  return IA_OK;
}

// ---- LPIPS head ----------------------------------------------------------------------------------------------------------------------
// A workgroup of 256 threads takes PXL consecutive pixels of one image pair (PXL = 16, or the power of two >= HW below that): PXL
// threads per pixel row, the 256 / PXL thread groups share the channels.  A pixel's sums over the groups, the workgroup's sum over its
// pixels and (second launch) the pair's sum over its workgroups are added in a fixed order.  The backward needs no sum across pixels.
#define HD_THREADS 256
#define HD_PIXELS 16

__device__ __forceinline__ float hd_group_sum(float *buf, int t, int pl, int PXL, float v) {
  buf[t] = v;
  __syncthreads();
  float s = 0.f;
  for (int g = 0; g < HD_THREADS / PXL; g++) s = s + buf[g * PXL + pl];
  __syncthreads();
  return s;
}

template <bool BWD>
__global__ __launch_bounds__(HD_THREADS) void k_lpips_head(const float *__restrict__ feat, const float *__restrict__ lin, int n, int C, int HW,
                                                           int PXL, int shift, int accumulate, float *__restrict__ out) {
  __shared__ float buf[HD_THREADS];
  const int i = blockIdx.x, t = threadIdx.x, pl = t & (PXL - 1), cg = t >> shift, CG = HD_THREADS / PXL;
  const float *a = feat + (size_t)i * C * HW, *b = feat + (size_t)(n + i) * C * HW;
  const float inv_hw = 1.f / (float)HW;
  const int r = blockIdx.y * PXL + pl;
  const bool ok = r < HW;
  float sa = 0.f, sb = 0.f;
  if (ok)
    for (int c = cg; c < C; c += CG) {
      const float av = a[(size_t)c * HW + r], bv = b[(size_t)c * HW + r];
      sa = __builtin_fmaf(av, av, sa);
      sb = __builtin_fmaf(bv, bv, sb);
    }
  const float SA = hd_group_sum(buf, t, pl, PXL, sa), SB = hd_group_sum(buf, t, pl, PXL, sb);
  const float ra = sqrtf(SA), na = ra + 1e-10f, nb = sqrtf(SB) + 1e-10f;
  float d = 0.f;
  if (ok)
    for (int c = cg; c < C; c += CG) {
      const float av = a[(size_t)c * HW + r], u = av / na - b[(size_t)c * HW + r] / nb;
      if (BWD) d = __builtin_fmaf(2.f * lin[c] * u * inv_hw, av, d);    // sum_c q_c a_c, q_c = 2 lin_c u_c / HW
      else d = __builtin_fmaf(lin[c], u * u, d);
    }
  const float D = hd_group_sum(buf, t, pl, PXL, d);
  if (BWD) {
    const float coef = SA > 0.f ? D / (na * na * ra) : 0.f;
    if (ok)
      for (int c = cg; c < C; c += CG) {
        const float av = a[(size_t)c * HW + r], u = av / na - b[(size_t)c * HW + r] / nb;
        const float q = 2.f * lin[c] * u * inv_hw, gr = q / na - coef * av;
        float *o = out + ((size_t)i * C + c) * HW + r;
        *o = accumulate ? *o + gr : gr;
      }
  } else {
    // the workgroup's pixels, in a fixed order: out = partial sums [n][gridDim.y]
    buf[t] = (ok && cg == 0) ? D : 0.f;
    __syncthreads();
    for (int o = HD_THREADS / 2; o > 0; o >>= 1) {
      if (t < o) buf[t] = buf[t] + buf[t + o];
      __syncthreads();
    }
    if (t == 0) out[(size_t)i * gridDim.y + blockIdx.y] = buf[0];
  }
}

__global__ void k_lpips_head_sum(const float *__restrict__ part, int n, int B, int HW, int accumulate, float *__restrict__ value) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int b = 0; b < B; b++) s = s + part[(size_t)i * B + b];
  const float r = s * (1.f / (float)HW);
  value[i] = accumulate ? value[i] + r : r;
}

static inline void head_geometry(int HW, int *PXL, int *shift) {
  int p = 1, s = 0;
  while (p < HW && p < HD_PIXELS) { p <<= 1; s++; }
  *PXL = p; *shift = s;
}

static inline bool head_shape_ok(int n, int C, int HW) {
  return n >= 1 && C >= 1 && HW >= 1 && (long long)C * HW < (1LL << 31) && (long long)2 * n * C * HW < (1LL << 31) &&
         (HW + HD_PIXELS - 1) / HD_PIXELS <= 65535;
}

extern "C" size_t ia_lpips_head_workspace_bytes(int n, int HW) {
  if (n < 1 || HW < 1 || (HW + HD_PIXELS - 1) / HD_PIXELS > 65535) return 0;
  int PXL, shift;
  head_geometry(HW, &PXL, &shift);
  return ia_align((size_t)n * ((HW + PXL - 1) / PXL) * sizeof(float));
}

extern "C" int ia_lpips_head(const float *feat, const float *lin, int n, int C, int HW, int accumulate, float *value, void *ws, size_t ws_bytes,
                             void *stream) {
  IA_CHECK_ARG(head_shape_ok(n, C, HW), "ia_lpips_head: n %d, C %d, HW %d: all >= 1, 2 n C HW < 2^31, HW <= 16 * 65535", n, C, HW);
  IA_CHECK_ARG(feat && lin && value, "ia_lpips_head: feat, lin and value are required");
  const size_t need = ia_lpips_head_workspace_bytes(n, HW);
  IA_CHECK_ARG(ws && ws_bytes >= need && ((uintptr_t)ws & 3) == 0, "ia_lpips_head: workspace of %zu bytes, %zu needed (ia_lpips_head_workspace_bytes)",
               ws_bytes, need);
  int PXL, shift;
  head_geometry(HW, &PXL, &shift);
  const int B = (HW + PXL - 1) / PXL;
  hipLaunchKernelGGL(k_lpips_head<false>, dim3(n, B), dim3(HD_THREADS), 0, (hipStream_t)stream, feat, lin, n, C, HW, PXL, shift, 0, (float *)ws);
  IA_LAUNCH_CHECK("k_lpips_head");
  hipLaunchKernelGGL(k_lpips_head_sum, dim3(ia_div_up(n, 64)), dim3(64), 0, (hipStream_t)stream, (const float *)ws, n, B, HW, accumulate ? 1 : 0,
                     value);
  IA_LAUNCH_CHECK("k_lpips_head_sum");
  return IA_OK;
}

extern "C" int ia_lpips_head_bwd(const float *feat, const float *lin, int n, int C, int HW, int accumulate, float *d_feat, void *stream) {
  IA_CHECK_ARG(head_shape_ok(n, C, HW), "ia_lpips_head_bwd: n %d, C %d, HW %d: all >= 1, 2 n C HW < 2^31, HW <= 16 * 65535", n, C, HW);
  IA_CHECK_ARG(feat && lin && d_feat, "ia_lpips_head_bwd: feat, lin and d_feat are required");
  int PXL, shift;
  head_geometry(HW, &PXL, &shift);
  hipLaunchKernelGGL(k_lpips_head<true>, dim3(n, (HW + PXL - 1) / PXL), dim3(HD_THREADS), 0, (hipStream_t)stream, feat, lin, n, C, HW, PXL, shift,
                     accumulate ? 1 : 0, d_feat);
  IA_LAUNCH_CHECK("k_lpips_head_bwd");
  return IA_OK;
}

// ---- depth regulariser ----------------------------------------------------------------------------------------------------------------
#define DR_THREADS 256

__device__ __forceinline__ double dr_block_sum(double *buf, int t, double v) {
  buf[t] = v;
  __syncthreads();
  for (int o = DR_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) buf[t] = buf[t] + buf[t + o];
    __syncthreads();
  }
  const double s = buf[0];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(DR_THREADS) void k_patch_depth_reg(const float *__restrict__ alpha, const float *__restrict__ depth, int n_patch,
                                                                int PQ, float *__restrict__ value, float *__restrict__ d_alpha,
                                                                float *__restrict__ d_depth) {
  __shared__ double buf[DR_THREADS];
  const int t = threadIdx.x;
  const double inv_tot = 1.0 / ((double)n_patch * (double)PQ);
  double vtot = 0.0;
  for (int p = 0; p < n_patch; p++) {
    const float *al = alpha + (size_t)p * PQ, *de = depth + (size_t)p * PQ;
    double sa = 0.0, sb = 0.0;
    for (int j = t; j < PQ; j += DR_THREADS) {
      const double a = al[j], d = de[j];
      sa = sa + a;
      sb = sb + d * a;
    }
    const double A = dr_block_sum(buf, t, sa) + 1e-3, B = dr_block_sum(buf, t, sb), avg = B / A;
    double st = 0.0, sv = 0.0;
    for (int j = t; j < PQ; j += DR_THREADS) {
      const double a = al[j], e = (double)de[j] - avg, sg = e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0);
      st = st + a * sg;
      sv = sv + a * fabs(e);
    }
    const double T = dr_block_sum(buf, t, st), V = dr_block_sum(buf, t, sv);
    vtot = vtot + V;
    for (int j = t; j < PQ; j += DR_THREADS) {
      const double a = al[j], e = (double)de[j] - avg, sg = e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0);
      d_depth[(size_t)p * PQ + j] = (float)((a * sg - T * a / A) * inv_tot);
      d_alpha[(size_t)p * PQ + j] = (float)((fabs(e) - T * e / A) * inv_tot);
    }
  }
  if (t == 0) value[0] = (float)(vtot * inv_tot);
}

extern "C" int ia_patch_depth_reg(const float *alpha, const float *depth, int n_patch, int PQ, float *value, float *d_alpha, float *d_depth,
                                  void *stream) {
  IA_CHECK_ARG(n_patch >= 1 && PQ >= 1 && (long long)n_patch * PQ < (1LL << 31), "ia_patch_depth_reg: n_patch %d, PQ %d: >= 1, n_patch PQ < 2^31",
               n_patch, PQ);
  IA_CHECK_ARG(alpha && depth && value && d_alpha && d_depth, "ia_patch_depth_reg: alpha, depth, value, d_alpha and d_depth are required");
  hipLaunchKernelGGL(k_patch_depth_reg, dim3(1), dim3(DR_THREADS), 0, (hipStream_t)stream, alpha, depth, n_patch, PQ, value, d_alpha, d_depth);
  IA_LAUNCH_CHECK("k_patch_depth_reg");
  return IA_OK;
}
