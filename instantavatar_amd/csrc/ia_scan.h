// ia_scan.h -- offsets out of counts, for the mesh units (ia_isosurface, ia_meshops, ia_meshdist): the exclusive prefix sum of one
// int32 per element over a whole array, and the int32 fill that clears the counts.  All sums are integer sums, so their order is fixed
// and so is every result.
//   the scan is three launches: per-workgroup sums (ia_block_combine, total only), one workgroup's scan over those sums
//   (k_scan_sums, whose carry loop takes a second trip past 1 024 workgroups = 262 144 elements), and the in-workgroup scan added
//   back.  A unit that has the count at hand fuses the first launch into its own pass (k_iso_mark) and uses the pieces.
// Everything has internal linkage: every unit that includes the header compiles its own copy of the kernels it launches.
#pragma once
#include "ia_common.h"

#define IA_SCAN_THREADS 256
#define IA_SCAN_WAVES (IA_SCAN_THREADS / 64)

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// one workgroup of IA_SCAN_THREADS lanes
// ---------------------------------------------------------------------------------------------------------------------
// x = the lane's exclusive prefix inside its wave, wave_total = the wave's sum -> the prefix over the workgroup, and the workgroup's
// total.  s_w: IA_SCAN_WAVES ints of LDS that nobody still reads (a kernel that scans twice puts a barrier in between); every lane
// of the workgroup has to come here: there is a barrier inside.
__device__ __forceinline__ int ia_block_combine(int x, int wave_total, int *s_w, int &total) {
  const int wave = threadIdx.x >> 6;
  if (ia_lane() == 0) s_w[wave] = wave_total;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < IA_SCAN_WAVES; w++) {
    if (w < wave) base += s_w[w];
    total += s_w[w];
  }
  return base + x;
}
// exclusive prefix sum of v over the workgroup
__device__ __forceinline__ int ia_block_excl_scan(int v, int *s_w, int &total) {
  int wave_total;
  const int x = ia_wave_excl_scan(v, wave_total);
  return ia_block_combine(x, wave_total, s_w, total);
}
// the same for v = flag ? 1 : 0, the index of a kept element among the kept ones: a ballot and two popcounts instead of the shuffles
__device__ __forceinline__ int ia_block_rank(bool flag, int *s_w, int &total) {
  const unsigned long long m = __ballot(flag);
  return ia_block_combine(__popcll(m & ((1ull << ia_lane()) - 1ull)), __popcll(m), s_w, total);
}

// ---------------------------------------------------------------------------------------------------------------------
// a whole array
// ---------------------------------------------------------------------------------------------------------------------
// n workgroup sums, scanned in place (exclusive); their total goes to total and total2 (either may be null)
struct ScanSums { int32_t *a; int n; int32_t *total, *total2; };

// workgroup b of the launch (1 024 lanes) takes array b: one launch scans one array or two
__global__ __launch_bounds__(1024) void k_scan_sums(ScanSums s0, ScanSums s1) {
  __shared__ int s_w[16];
  const ScanSums S = blockIdx.x == 0 ? s0 : s1;
  const int wave = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < S.n; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < S.n ? S.a[i] : 0;
    int wave_total;
    const int x = ia_wave_excl_scan(v, wave_total);
    if (ia_lane() == 0) s_w[wave] = wave_total;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) {
      if (w < wave) before += s_w[w];
      total += s_w[w];
    }
    if (i < S.n) S.a[i] = carry + before + x;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (S.total) *S.total = carry;
    if (S.total2) *S.total2 = carry;
  }
}
inline void ia_scan_sums(ScanSums s0, hipStream_t s) { hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, s, s0, ScanSums{nullptr, 0, nullptr, nullptr}); }
inline void ia_scan_sums(ScanSums s0, ScanSums s1, hipStream_t s) { hipLaunchKernelGGL(k_scan_sums, dim3(2), dim3(1024), 0, s, s0, s1); }

// what is counted per element
struct LoadInt {
  const int32_t *p;
  __device__ __forceinline__ int operator()(long long i) const { return p[i]; }
};
struct LoadPopc {
  const uint32_t *p;
  __device__ __forceinline__ int operator()(long long i) const { return __popc(p[i]); }
};

template <class L>
__global__ __launch_bounds__(IA_SCAN_THREADS) void k_scan_block_sums(L load, long long n, int32_t *__restrict__ bsum) {
  __shared__ int s_w[IA_SCAN_WAVES];
  const long long i = (long long)blockIdx.x * IA_SCAN_THREADS + threadIdx.x;
  int v = i < n ? load(i) : 0, total;                      // (only the total is wanted: the wave's sum by a butterfly, no prefixes)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  ia_block_combine(0, v, s_w, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
template <class L>
__global__ __launch_bounds__(IA_SCAN_THREADS) void k_scan_block_scan(L load, long long n, const int32_t *__restrict__ bsum,
                                                                     int32_t *__restrict__ start) {
  __shared__ int s_w[IA_SCAN_WAVES];
  const long long i = (long long)blockIdx.x * IA_SCAN_THREADS + threadIdx.x;
  int total;
  const int x = ia_block_excl_scan(i < n ? load(i) : 0, s_w, total);
  if (i < n) start[i] = bsum[blockIdx.x] + x;
}

// start[i] = sum of load(j) over j < i, i = 0 .. n (n >= 1); bsum: ia_div_up(n, IA_SCAN_THREADS) ints of scratch; total: also
// written there (or null)
template <class L>
void ia_scan(L load, long long n, int32_t *bsum, int32_t *start, int32_t *total, hipStream_t s) {
  const int nb = ia_div_up(n, IA_SCAN_THREADS);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_block_sums<L>), dim3(nb), dim3(IA_SCAN_THREADS), 0, s, load, n, bsum);
  ia_scan_sums(ScanSums{bsum, nb, start + n, total}, s);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_block_scan<L>), dim3(nb), dim3(IA_SCAN_THREADS), 0, s, load, n, (const int32_t *)bsum, start);
}

__global__ __launch_bounds__(IA_SCAN_THREADS) void k_fill_i32(int32_t *__restrict__ p, long long n, int32_t value) {
  const long long i = (long long)blockIdx.x * IA_SCAN_THREADS + threadIdx.x;
  if (i < n) p[i] = value;
}
inline void ia_fill_i32(int32_t *p, long long n, int32_t value, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_fill_i32, dim3(ia_div_up(n, IA_SCAN_THREADS)), dim3(IA_SCAN_THREADS), 0, s, p, n, value);
}

}  // namespace
