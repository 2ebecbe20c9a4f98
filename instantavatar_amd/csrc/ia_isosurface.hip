// ia_isosurface.hip -- triangle meshes out of the density field (no counterpart in the reference, whose helper is marching
// cubes on the host): the isosurface of a scalar lattice by marching tetrahedra, the largest connected component of a
// mesh, per-vertex normals from gradients and forward skinning of canonical points.
//   lattice positions, in chunks, for the field                                  (ia_iso_lattice_points)
//   classify, mark owned crossing edges, count triangles, both prefix sums       (ia_iso_count)
//   vertices and faces in the order the definition fixes                         (ia_iso_emit)
//   union-find over the faces, areas in 64-bit fixed point, order-preserving compaction   (ia_mesh_largest_count / _emit)
//   n = -g / |g|                                                                  (ia_unit_negative)
//   x_d = s2w (J(x_c) [x_c; 1])                                                   (ia_forward_skin)
// The definition is stated in DESIGN.md section 4 and in include/instantavatar_hip_mesh.h.  Nothing here synchronises,
// allocates or reads on the host; every pass is streaming and memory bound.
//
// One lane = one lattice point, z fastest: the point owns the (up to) 7 edges towards the other corners of the cell whose
// origin it is, and the lane handles that cell as well, so the eight corner loads of neighbouring lanes coalesce and cell
// order = point order.  Counts are turned into offsets by the three launches of ia_scan.h, the first of them fused into the marking
// pass (k_iso_mark has both counts of a point at hand); the face pieces of the component pass come from ia_mesh_dev.h.
#include "ia_common.h"
#include "ia_mesh_dev.h"
#include "ia_scan.h"
#include "ia_search_dev.h"
#include "../../include/instantavatar_hip_mesh.h"
#define IA_MT_QUAL static __device__ const
#include "ia_mt_table.h"

#define IA_ISO_THREADS IA_SCAN_THREADS
#define IA_ISO_WAVES IA_SCAN_WAVES

struct IsoBox { float lo[3], hi[3]; };

// ---------------------------------------------------------------------------------------------------------------------
// lattice
// ---------------------------------------------------------------------------------------------------------------------
// position of sample i of N along one axis: lo + (hi - lo) * (i / (N - 1)), every operation rounded to fp32 on its own
__device__ __forceinline__ float iso_coord(float lo, float hi, int i, int N) {
  return lo + (hi - lo) * ((float)i / (float)(N - 1));
}

__global__ __launch_bounds__(256) void k_iso_points(IsoBox B, int N, long long first, int count, float *__restrict__ pts) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const long long p = first + t;
  const int k = (int)(p % N), j = (int)(p / N % N), i = (int)(p / ((long long)N * N));
  pts[(size_t)t * 3] = iso_coord(B.lo[0], B.hi[0], i, N);
  pts[(size_t)t * 3 + 1] = iso_coord(B.lo[1], B.hi[1], j, N);
  pts[(size_t)t * 3 + 2] = iso_coord(B.lo[2], B.hi[2], k, N);
}

static int iso_check_lattice(const ia_occ_grid *lattice, const char *who, IsoBox *B) {
  IA_CHECK_ARG(lattice, "%s: null lattice", who);
  IA_CHECK_ARG(lattice->G >= 2 && lattice->G <= IA_ISO_MAX_N, "%s: N = %d outside [2, %d]", who, lattice->G, IA_ISO_MAX_N);
  for (int d = 0; d < 3; d++) { B->lo[d] = lattice->aabb_min[d]; B->hi[d] = lattice->aabb_max[d]; }
  return IA_OK;
}

extern "C" int ia_iso_lattice_points(const ia_occ_grid *lattice, long long first, int count, float *pts, void *stream) {
  IsoBox B;
  const int rc = iso_check_lattice(lattice, "ia_iso_lattice_points", &B);
  if (rc) return rc;
  const long long n = (long long)lattice->G * lattice->G * lattice->G;
  IA_CHECK_ARG(first >= 0 && count >= 0 && first + count <= n, "ia_iso_lattice_points: points %lld .. +%d outside the lattice", first, count);
  if (count == 0) return IA_OK;
  IA_CHECK_ARG(pts, "ia_iso_lattice_points: null pointer");
  hipLaunchKernelGGL(k_iso_points, dim3(ia_div_up(count, 256)), dim3(256), 0, (hipStream_t)stream, B, lattice->G, first, count, pts);
  IA_LAUNCH_CHECK("k_iso_points");
  return IA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// marching tetrahedra
// ---------------------------------------------------------------------------------------------------------------------
// the scalar of lattice point (i, j, k): a non-finite sample counts as 0, and with `cap` so does the outermost layer
__device__ __forceinline__ float iso_scalar(const float *__restrict__ sigma, int N, int i, int j, int k, int cap) {
  if (cap && (i == 0 || j == 0 || k == 0 || i == N - 1 || j == N - 1 || k == N - 1)) return 0.f;
  const float s = sigma[((long long)i * N + j) * N + k];
  return __builtin_fabsf(s) < INFINITY ? s : 0.f;
}

// what a lane knows about its point p = (i, j, k): `in` = bit c set when corner c = 4 x + 2 y + z of the cell with origin p
// lies in the lattice and is inside; `have` = bit c set when the corner lies in the lattice
struct IsoCell { int i, j, k; uint32_t in, have; };

__device__ __forceinline__ bool iso_cell(const float *__restrict__ sigma, int N, float level, int cap, long long p, long long n, IsoCell &c) {
  c.in = c.have = 0u;
  c.i = c.j = c.k = 0;
  if (p >= n) return false;
  c.k = (int)(p % N); c.j = (int)(p / N % N); c.i = (int)(p / ((long long)N * N));
#pragma unroll
  for (int q = 0; q < 8; q++) {
    const int ii = c.i + (q >> 2), jj = c.j + ((q >> 1) & 1), kk = c.k + (q & 1);
    if (ii < N && jj < N && kk < N) {
      c.have |= 1u << q;
      if (iso_scalar(sigma, N, ii, jj, kk, cap) > level) c.in |= 1u << q;
    }
  }
  return true;
}

// the crossing edges the point owns: bit s set for slot s.  Slot s points at corner IA_SLOT_CORNER(s) of the point's cell.
__device__ __forceinline__ int iso_slot_corner(int s) {   // (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1)
  return (0x7356124 >> (4 * s)) & 7;                        // corners 4, 2, 1, 6, 5, 3, 7
}
__device__ __forceinline__ uint32_t iso_owned_edges(const IsoCell &c) {
  uint32_t m = 0u;
  const uint32_t self = c.in & 1u;
#pragma unroll
  for (int s = 0; s < 7; s++) {
    const int q = iso_slot_corner(s);
    if (((c.have >> q) & 1u) && ((c.in >> q) & 1u) != self) m |= 1u << s;
  }
  return m;
}

// the 4-bit case of tetrahedron t
__device__ __forceinline__ int iso_case(uint32_t in, int t) {
  int cs = 0;
#pragma unroll
  for (int v = 0; v < 4; v++) cs |= (int)((in >> IA_MT_CORNER[t][v]) & 1u) << v;
  return cs;
}

// triangles of the cell: 1 for one or three inside vertices of a tetrahedron, 2 for two (= IA_MT_NTRI)
__device__ __forceinline__ int iso_cell_triangles(const IsoCell &c) {
  if (c.have != 0xffu || c.in == 0u || c.in == 0xffu) return 0;
  int n = 0;
#pragma unroll
  for (int t = 0; t < 6; t++) n += IA_MT_NTRI[t][iso_case(c.in, t)];
  return n;
}

__global__ __launch_bounds__(IA_ISO_THREADS) void k_iso_mark(const float *__restrict__ sigma, int N, float level, int cap,
                                                             uint8_t *__restrict__ vmask, int32_t *__restrict__ vsum,
                                                             int32_t *__restrict__ fsum) {
  __shared__ int s_v[IA_ISO_WAVES], s_f[IA_ISO_WAVES];
  const long long n = (long long)N * N * N;
  const long long p = (long long)blockIdx.x * IA_ISO_THREADS + threadIdx.x;
  IsoCell c;
  const bool live = iso_cell(sigma, N, level, cap, p, n, c);
  const uint32_t m = iso_owned_edges(c);
  if (live) vmask[p] = (uint8_t)m;
  int nv = __popc(m), nf = iso_cell_triangles(c);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { nv += __shfl_xor(nv, o, 64); nf += __shfl_xor(nf, o, 64); }
  if (ia_lane() == 0) { s_v[threadIdx.x >> 6] = nv; s_f[threadIdx.x >> 6] = nf; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int a = 0, b = 0;
#pragma unroll
    for (int w = 0; w < IA_ISO_WAVES; w++) { a += s_v[w]; b += s_f[w]; }
    vsum[blockIdx.x] = a;
    fsum[blockIdx.x] = b;
  }
}

// vbase[p] = index of the first vertex the point owns
__global__ __launch_bounds__(IA_ISO_THREADS) void k_iso_vbase(const uint8_t *__restrict__ vmask, long long n, const int32_t *__restrict__ vsum,
                                                              int32_t *__restrict__ vbase) {
  __shared__ int s_w[IA_ISO_WAVES];
  const long long p = (long long)blockIdx.x * IA_ISO_THREADS + threadIdx.x;
  int total;
  const int x = ia_block_excl_scan(p < n ? __popc((uint32_t)vmask[p]) : 0, s_w, total);
  if (p < n) vbase[p] = vsum[blockIdx.x] + x;
}

__global__ __launch_bounds__(IA_ISO_THREADS) void k_iso_verts(const float *__restrict__ sigma, IsoBox B, int N, float level, int cap,
                                                              const uint8_t *__restrict__ vmask, const int32_t *__restrict__ vbase,
                                                              float *__restrict__ verts, int nv_cap) {
  const long long n = (long long)N * N * N;
  const long long p = (long long)blockIdx.x * IA_ISO_THREADS + threadIdx.x;
  if (p >= n) return;
  const uint32_t m = vmask[p];
  if (m == 0u) return;
  const int k = (int)(p % N), j = (int)(p / N % N), i = (int)(p / ((long long)N * N));
  const float sa = iso_scalar(sigma, N, i, j, k, cap);
  const float pa[3] = {iso_coord(B.lo[0], B.hi[0], i, N), iso_coord(B.lo[1], B.hi[1], j, N), iso_coord(B.lo[2], B.hi[2], k, N)};
  int at = vbase[p];
  for (int s = 0; s < 7; s++) {
    if (!((m >> s) & 1u)) continue;
    const int q = iso_slot_corner(s);
    const int ii = i + (q >> 2), jj = j + ((q >> 1) & 1), kk = k + (q & 1);   // in the lattice: the edge was marked
    const float sb = iso_scalar(sigma, N, ii, jj, kk, cap);
    const float pb[3] = {iso_coord(B.lo[0], B.hi[0], ii, N), iso_coord(B.lo[1], B.hi[1], jj, N), iso_coord(B.lo[2], B.hi[2], kk, N)};
    const float t = (level - sa) / (sb - sa);       // the edge crosses: sa != sb
    if ((uint32_t)at < (uint32_t)nv_cap) {
#pragma unroll
      for (int d = 0; d < 3; d++) verts[(size_t)at * 3 + d] = __builtin_fmaf(t, pb[d] - pa[d], pa[d]);
    }
    at++;
  }
}

__global__ __launch_bounds__(IA_ISO_THREADS) void k_iso_faces(const float *__restrict__ sigma, int N, float level, int cap,
                                                              const uint8_t *__restrict__ vmask, const int32_t *__restrict__ vbase,
                                                              const int32_t *__restrict__ fsum, int32_t *__restrict__ faces, int nf_cap) {
  __shared__ int s_w[IA_ISO_WAVES];
  __shared__ uint8_t s_edge[6 * 16 * 6];
  for (int e = threadIdx.x; e < 6 * 16 * 6; e += IA_ISO_THREADS) s_edge[e] = (&IA_MT_EDGE[0][0][0])[e];
  const long long n = (long long)N * N * N;
  const long long p = (long long)blockIdx.x * IA_ISO_THREADS + threadIdx.x;
  IsoCell c;
  iso_cell(sigma, N, level, cap, p, n, c);
  const int nf = iso_cell_triangles(c);
  int total;
  int at = fsum[blockIdx.x] + ia_block_excl_scan(nf, s_w, total);   // (the scan's barrier also publishes s_edge)
  if (nf == 0) return;
  for (int t = 0; t < 6; t++) {
    const int cs = iso_case(c.in, t);
    const int nt = IA_MT_NTRI[t][cs];
    for (int tri = 0; tri < nt; tri++) {
      int32_t v[3];
#pragma unroll
      for (int e = 0; e < 3; e++) {
        const uint32_t code = s_edge[(t * 16 + cs) * 6 + 3 * tri + e];
        const uint32_t q = code >> 3, slot = code & 7u;
        const long long owner = p + ((long long)(q >> 2) * N + ((q >> 1) & 1u)) * N + (q & 1u);   // a corner of a whole cell
        v[e] = vbase[owner] + __popc((uint32_t)vmask[owner] & ((1u << slot) - 1u));
      }
      if ((uint32_t)at < (uint32_t)nf_cap) {
#pragma unroll
        for (int e = 0; e < 3; e++) faces[(size_t)at * 3 + e] = v[e];
      }
      at++;
    }
  }
}

struct IsoWs { uint8_t *vmask; int32_t *vbase, *vsum, *fsum; size_t bytes; int blocks; };
static IsoWs iso_carve(void *ws, int N) {
  const size_t n = (size_t)N * N * N;
  WsCarver w(ws, 0);
  IsoWs o;
  o.blocks = (int)((n + IA_ISO_THREADS - 1) / IA_ISO_THREADS);
  o.vmask = w.take<uint8_t>(n);
  o.vbase = w.take<int32_t>(n);
  o.vsum = w.take<int32_t>(o.blocks);
  o.fsum = w.take<int32_t>(o.blocks);
  o.bytes = w.off;
  return o;
}

extern "C" size_t ia_iso_workspace_bytes(int N) {
  if (N < 2 || N > IA_ISO_MAX_N) return 0;
  return iso_carve(nullptr, N).bytes;
}

extern "C" int ia_iso_count(const float *sigma, int N, float level, int cap, void *ws, size_t ws_bytes, int32_t *counts, void *stream) {
  IA_CHECK_ARG(N >= 2 && N <= IA_ISO_MAX_N, "ia_iso_count: N = %d outside [2, %d]", N, IA_ISO_MAX_N);
  IA_CHECK_ARG(sigma && ws && counts, "ia_iso_count: null pointer");
  IA_CHECK_ARG(level == level, "ia_iso_count: the level is NaN");
  const IsoWs W = iso_carve(ws, N);
  if (ws_bytes < W.bytes) return ia_set_error(IA_ERR_WORKSPACE, "ia_iso_count: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const long long n = (long long)N * N * N;
  hipLaunchKernelGGL(k_iso_mark, dim3(W.blocks), dim3(IA_ISO_THREADS), 0, s, sigma, N, level, cap, W.vmask, W.vsum, W.fsum);
  ia_scan_sums(ScanSums{W.vsum, W.blocks, counts, nullptr}, ScanSums{W.fsum, W.blocks, counts + 1, nullptr}, s);
  hipLaunchKernelGGL(k_iso_vbase, dim3(W.blocks), dim3(IA_ISO_THREADS), 0, s, W.vmask, n, W.vsum, W.vbase);
  IA_LAUNCH_CHECK("k_iso_vbase");
  return IA_OK;
}

extern "C" int ia_iso_emit(const float *sigma, const ia_occ_grid *lattice, float level, int cap, const void *ws, size_t ws_bytes,
                           float *verts, int nv, int32_t *faces, int nf, void *stream) {
  IsoBox B;
  const int rc = iso_check_lattice(lattice, "ia_iso_emit", &B);
  if (rc) return rc;
  IA_CHECK_ARG(nv >= 0 && nf >= 0, "ia_iso_emit: negative capacity");
  if (nv == 0 && nf == 0) return IA_OK;
  IA_CHECK_ARG(sigma && ws && (nv == 0 || verts) && (nf == 0 || faces), "ia_iso_emit: null pointer");
  const int N = lattice->G;
  const IsoWs W = iso_carve(const_cast<void *>(ws), N);
  if (ws_bytes < W.bytes) return ia_set_error(IA_ERR_WORKSPACE, "ia_iso_emit: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  if (nv > 0)
    hipLaunchKernelGGL(k_iso_verts, dim3(W.blocks), dim3(IA_ISO_THREADS), 0, s, sigma, B, N, level, cap, W.vmask, W.vbase, verts, nv);
  if (nf > 0)
    hipLaunchKernelGGL(k_iso_faces, dim3(W.blocks), dim3(IA_ISO_THREADS), 0, s, sigma, N, level, cap, W.vmask, W.vbase, W.fsum, faces, nf);
  IA_LAUNCH_CHECK("k_iso_faces");
  return IA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// largest connected component
// ---------------------------------------------------------------------------------------------------------------------
// Union-find over the vertices as in ia_render.hip (k_occ_union), mirrored: the root of a component is its SMALLEST vertex
// index, so parents only ever decrease -- a chain is strictly decreasing and ends, path compression is a monotone atomicMin
// that cannot undo a concurrent link, and the retry of a failed compare-and-swap follows another thread's completed link
// (lock-free: nobody waits for a thread that has yet to run).
struct CcHead { unsigned long long best_area; int32_t best_root; int32_t pad; };

__device__ __forceinline__ int cc_find(int32_t *parent, int i) {
  const int start = i;
  int p = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (p != i) { i = p; p = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  if (start != i) atomicMin(&parent[start], i);
  return i;
}

__device__ __forceinline__ void cc_union(int32_t *parent, int a, int b) {
  while (true) {
    a = cc_find(parent, a); b = cc_find(parent, b);
    if (a == b) break;
    if (a < b) { const int t = a; a = b; b = t; }
    if (atomicCAS(&parent[a], a, b) == a) break;   // link the larger root under the smaller
  }
}

__device__ __forceinline__ bool cc_face(const int32_t *__restrict__ faces, int f, int nv, int v[3]) {
  ia_face_load(faces, f, v);
  return ia_face_in_range(v, nv);   // others are ignored
}

__global__ __launch_bounds__(256) void k_cc_init(int32_t *__restrict__ parent, unsigned long long *__restrict__ area, int nv, CcHead *head) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v == 0) { head->best_area = 0ull; head->best_root = INT_MAX; head->pad = 0; }
  if (v >= nv) return;
  parent[v] = v;
  area[v] = 0ull;
}

__global__ __launch_bounds__(256) void k_cc_union(const int32_t *__restrict__ faces, int nf, int nv, int32_t *parent) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  int v[3];
  if (f >= nf || !cc_face(faces, f, nv, v)) return;
  cc_union(parent, v[0], v[1]);
  cc_union(parent, v[0], v[2]);
}

// area of a face in units of area_unit / 2^40, at least 1: a component that has a face has a positive area
__global__ __launch_bounds__(256) void k_cc_area(const float *__restrict__ verts, const int32_t *__restrict__ faces, int nf, int nv,
                                                 double scale, int32_t *parent, unsigned long long *area) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  int v[3];
  const bool ok = f < nf && cc_face(faces, f, nv, v);
  int root = -1;
  unsigned long long a = 0ull;
  if (ok) {
    root = cc_find(parent, v[0]);
    double p[3][3], c[3];
    ia_face_corners(verts, v, p);
    ia_face_cross(p, c);
    const double fixed = 0.5 * ia_len3d(c) * scale;
    a = fixed >= 1.0 && fixed < 4.0e18 ? (unsigned long long)fixed : 1ull;   // (tiny, NaN and overflowing areas count 1)
  }
  // most lanes of a wave belong to the same component: one atomic per wave then (integer sums: any order, the same total)
  const unsigned long long m = __ballot(ok);
  if (m == 0ull) return;
  const int first = __shfl(root, __ffsll((long long)m) - 1, 64);
  if (__all(!ok || root == first)) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (ia_lane() == __ffsll((long long)m) - 1) atomicAdd(&area[first], a);
  } else if (ok) {
    atomicAdd(&area[root], a);
  }
}

// the largest area over the roots, then the smallest root that has it
__global__ __launch_bounds__(256) void k_cc_best_area(const int32_t *__restrict__ parent, const unsigned long long *__restrict__ area,
                                                      int nv, CcHead *head) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long a = (v < nv && parent[v] == v) ? area[v] : 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long b = __shfl_xor(a, o, 64); a = b > a ? b : a; }
  if (ia_lane() == 0 && a > 0ull) atomicMax(&head->best_area, a);
}
__global__ __launch_bounds__(256) void k_cc_best_root(const int32_t *__restrict__ parent, const unsigned long long *__restrict__ area,
                                                      int nv, CcHead *head) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv || parent[v] != v) return;
  const unsigned long long a = area[v];
  if (a > 0ull && a == head->best_area) atomicMin(&head->best_root, v);
}

// thread i: is vertex i kept, is face i kept; per-workgroup counts
__device__ __forceinline__ bool cc_keep_vertex(int32_t *parent, int v, int nv, int best) { return v < nv && cc_find(parent, v) == best; }
__device__ __forceinline__ bool cc_keep_face(const int32_t *__restrict__ faces, const int32_t *__restrict__ vnew, int f, int nf, int nv, int v[3]) {
  return f < nf && cc_face(faces, f, nv, v) && vnew[v[0]] >= 0;
}
// (the index of a kept element among the kept elements of its workgroup, and their number: ia_block_rank)

__global__ __launch_bounds__(256) void k_cc_count_verts(int32_t *parent, int nv, const CcHead *__restrict__ head, int32_t *__restrict__ vsum) {
  __shared__ int s_w[4];
  const int v = blockIdx.x * 256 + threadIdx.x;
  int c;
  ia_block_rank(cc_keep_vertex(parent, v, nv, head->best_root), s_w, c);
  if (threadIdx.x == 0) vsum[blockIdx.x] = c;
}
__global__ __launch_bounds__(256) void k_cc_index_verts(int32_t *parent, int nv, const CcHead *__restrict__ head, const int32_t *__restrict__ vsum,
                                                        int32_t *__restrict__ vnew) {
  __shared__ int s_w[4];
  const int v = blockIdx.x * 256 + threadIdx.x;
  const bool keep = cc_keep_vertex(parent, v, nv, head->best_root);
  int c;
  const int r = ia_block_rank(keep, s_w, c);
  if (v < nv) vnew[v] = keep ? vsum[blockIdx.x] + r : -1;
}
__global__ __launch_bounds__(256) void k_cc_count_faces(const int32_t *__restrict__ faces, int nf, int nv, const int32_t *__restrict__ vnew,
                                                        int32_t *__restrict__ fsum) {
  __shared__ int s_w[4];
  const int f = blockIdx.x * 256 + threadIdx.x;
  int v[3], c;
  ia_block_rank(cc_keep_face(faces, vnew, f, nf, nv, v), s_w, c);
  if (threadIdx.x == 0) fsum[blockIdx.x] = c;
}

__global__ __launch_bounds__(256) void k_cc_emit_verts(const float *__restrict__ verts, int nv, const int32_t *__restrict__ vnew,
                                                       float *__restrict__ verts_out, int32_t *__restrict__ vert_src, int cap) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const int k = vnew[v];
  if ((uint32_t)k >= (uint32_t)cap) return;      // dropped (-1) or past the buffer
#pragma unroll
  for (int d = 0; d < 3; d++) verts_out[(size_t)k * 3 + d] = verts[(size_t)v * 3 + d];
  if (vert_src) vert_src[k] = v;
}
__global__ __launch_bounds__(256) void k_cc_emit_faces(const int32_t *__restrict__ faces, int nf, int nv, const int32_t *__restrict__ vnew,
                                                       const int32_t *__restrict__ fsum, int32_t *__restrict__ faces_out, int cap) {
  __shared__ int s_w[4];
  const int f = blockIdx.x * 256 + threadIdx.x;
  int v[3], c;
  const bool keep = cc_keep_face(faces, vnew, f, nf, nv, v);
  const int k = fsum[blockIdx.x] + ia_block_rank(keep, s_w, c);
  if (!keep || (uint32_t)k >= (uint32_t)cap) return;
#pragma unroll
  for (int e = 0; e < 3; e++) faces_out[(size_t)k * 3 + e] = vnew[v[e]];
}

struct CcWs { CcHead *head; int32_t *parent, *vnew, *vsum, *fsum; unsigned long long *area; size_t bytes; int vblocks, fblocks; };
static CcWs cc_carve(void *ws, int nv, int nf) {
  WsCarver w(ws, 0);
  CcWs o;
  o.vblocks = ia_div_up(nv > 0 ? nv : 1, 256);
  o.fblocks = ia_div_up(nf > 0 ? nf : 1, 256);
  o.head = w.take<CcHead>(1);
  o.parent = w.take<int32_t>(nv);
  o.vnew = w.take<int32_t>(nv);
  o.area = w.take<unsigned long long>(nv);
  o.vsum = w.take<int32_t>(o.vblocks);
  o.fsum = w.take<int32_t>(o.fblocks);
  o.bytes = w.off;
  return o;
}

extern "C" size_t ia_mesh_component_workspace_bytes(int nv, int nf) {
  if (nv < 0 || nf < 0) return 0;
  return cc_carve(nullptr, nv, nf).bytes;
}

extern "C" int ia_mesh_largest_count(const float *verts, const int32_t *faces, int nv, int nf, float area_unit, void *ws, size_t ws_bytes,
                                     int32_t *counts, void *stream) {
  IA_CHECK_ARG(nv >= 0 && nf >= 0, "ia_mesh_largest_count: negative size");
  IA_CHECK_ARG(area_unit > 0.f && area_unit < INFINITY, "ia_mesh_largest_count: area_unit must be positive and finite");
  IA_CHECK_ARG(ws && counts && (nv == 0 || verts) && (nf == 0 || faces), "ia_mesh_largest_count: null pointer");
  const CcWs W = cc_carve(ws, nv, nf);
  if (ws_bytes < W.bytes) return ia_set_error(IA_ERR_WORKSPACE, "ia_mesh_largest_count: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const dim3 b(256), gv(W.vblocks), gf(W.fblocks);
  hipLaunchKernelGGL(k_cc_init, gv, b, 0, s, W.parent, W.area, nv, W.head);
  if (nf > 0 && nv > 0) {
    hipLaunchKernelGGL(k_cc_union, gf, b, 0, s, faces, nf, nv, W.parent);
    hipLaunchKernelGGL(k_cc_area, gf, b, 0, s, verts, faces, nf, nv, 1099511627776.0 / (double)area_unit, W.parent, W.area);
    hipLaunchKernelGGL(k_cc_best_area, gv, b, 0, s, W.parent, W.area, nv, W.head);
    hipLaunchKernelGGL(k_cc_best_root, gv, b, 0, s, W.parent, W.area, nv, W.head);
  }
  // (without a face nothing is kept: best_root stays INT_MAX)
  hipLaunchKernelGGL(k_cc_count_verts, gv, b, 0, s, W.parent, nv, W.head, W.vsum);
  ia_scan_sums(ScanSums{W.vsum, W.vblocks, counts, nullptr}, s);
  hipLaunchKernelGGL(k_cc_index_verts, gv, b, 0, s, W.parent, nv, W.head, W.vsum, W.vnew);
  hipLaunchKernelGGL(k_cc_count_faces, gf, b, 0, s, faces, nf, nv, W.vnew, W.fsum);
  ia_scan_sums(ScanSums{W.fsum, W.fblocks, counts + 1, nullptr}, s);
  IA_LAUNCH_CHECK("k_cc_count_faces");
  return IA_OK;
}

extern "C" int ia_mesh_largest_emit(const float *verts, const int32_t *faces, int nv, int nf, const void *ws, size_t ws_bytes,
                                    float *verts_out, int nv_out, int32_t *faces_out, int nf_out, int32_t *vert_src, void *stream) {
  IA_CHECK_ARG(nv >= 0 && nf >= 0 && nv_out >= 0 && nf_out >= 0, "ia_mesh_largest_emit: negative size");
  IA_CHECK_ARG(ws && (nv == 0 || verts) && (nf == 0 || faces) && (nv_out == 0 || verts_out) && (nf_out == 0 || faces_out),
               "ia_mesh_largest_emit: null pointer");
  const CcWs W = cc_carve(const_cast<void *>(ws), nv, nf);
  if (ws_bytes < W.bytes) return ia_set_error(IA_ERR_WORKSPACE, "ia_mesh_largest_emit: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  if (nv > 0 && nv_out > 0)
    hipLaunchKernelGGL(k_cc_emit_verts, dim3(W.vblocks), dim3(256), 0, s, verts, nv, W.vnew, verts_out, vert_src, nv_out);
  if (nf > 0 && nf_out > 0)
    hipLaunchKernelGGL(k_cc_emit_faces, dim3(W.fblocks), dim3(256), 0, s, faces, nf, nv, W.vnew, W.fsum, faces_out, nf_out);
  IA_LAUNCH_CHECK("k_cc_emit_faces");
  return IA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// normals of canonical vertices: n = -g / |g|, zero where g is zero or not finite
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_unit_negative(const float *__restrict__ g, int n, float *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float g0 = g[(size_t)i * 3], g1 = g[(size_t)i * 3 + 1], g2 = g[(size_t)i * 3 + 2];
  // scaled by the largest component first: the squares neither overflow nor underflow for any finite gradient
  const float gm = fmaxf(fmaxf(__builtin_fabsf(g0), __builtin_fabsf(g1)), __builtin_fabsf(g2));
  float u[3] = {0.f, 0.f, 0.f};
  if (gm < INFINITY && gm > 0.f && g0 == g0 && g1 == g1 && g2 == g2) {
    const float h0 = -g0 / gm, h1 = -g1 / gm, h2 = -g2 / gm;
    const float len = sqrtf(IA_DOT3(h0, h0, h1, h1, h2, h2));
    u[0] = h0 / len; u[1] = h1 / len; u[2] = h2 / len;
  }
#pragma unroll
  for (int d = 0; d < 3; d++) out[(size_t)i * 3 + d] = u[d];
}

extern "C" int ia_unit_negative(const float *g, int n, float *out, void *stream) {
  IA_CHECK_ARG(n >= 0, "ia_unit_negative: n < 0");
  if (n == 0) return IA_OK;
  IA_CHECK_ARG(g && out, "ia_unit_negative: null pointer");
  hipLaunchKernelGGL(k_unit_negative, dim3(ia_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, g, n, out);
  IA_LAUNCH_CHECK("k_unit_negative");
  return IA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// forward skinning: one lane = one canonical point.  J = the search's trilinear fetch of the 12-channel transform grid at
// x_c (fetch_plan: 8 corner records of 48 B, corners outside the grid with weight 0, accumulated in the reference's corner
// order), y = J [x_c; 1] in the SMPL-root frame, x_d = s2w [y; 1].  With every corner outside J = 0, y = 0 and x_d is s2w's
// translation exactly.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_forward_skin(const float *__restrict__ xc, int n, const float *__restrict__ voxel_J, SnarfGridDev G,
                                                      const float *__restrict__ s2w, float *__restrict__ xd) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const float x0 = xc[(size_t)p * 3], x1 = xc[(size_t)p * 3 + 1], x2 = xc[(size_t)p * 3 + 2];
  FetchPlan fp;
  fetch_plan(G, G.scl[0] * (x0 + G.off[0]), G.scl[1] * (x1 + G.off[1]), G.scl[2] * (x2 + G.off[2]), true, fp);
  float J[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (fp.load != 0) {
    const char *vJb = reinterpret_cast<const char *>(voxel_J);
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const float4 *rec = reinterpret_cast<const float4 *>(vJb + (size_t)fp.off[c]);
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const float4 v = rec[r];
        J[4 * r] = __builtin_fmaf(v.x, fp.w[c], J[4 * r]);
        J[4 * r + 1] = __builtin_fmaf(v.y, fp.w[c], J[4 * r + 1]);
        J[4 * r + 2] = __builtin_fmaf(v.z, fp.w[c], J[4 * r + 2]);
        J[4 * r + 3] = __builtin_fmaf(v.w, fp.w[c], J[4 * r + 3]);
      }
    }
  }
  float y[3];
#pragma unroll
  for (int r = 0; r < 3; r++) y[r] = IA_DOT3(J[4 * r], x0, J[4 * r + 1], x1, J[4 * r + 2], x2) + J[4 * r + 3];
#pragma unroll
  for (int d = 0; d < 3; d++) xd[(size_t)p * 3 + d] = IA_DOT3(s2w[4 * d], y[0], s2w[4 * d + 1], y[1], s2w[4 * d + 2], y[2]) + s2w[4 * d + 3];
}

extern "C" int ia_forward_skin(const float *xc, int n, const float *voxel_J, const ia_snarf_grid *grid, const float *s2w, float *xd,
                               void *stream) {
  IA_CHECK_ARG(n >= 0, "ia_forward_skin: n < 0");
  if (n == 0) return IA_OK;
  IA_CHECK_ARG(xc && voxel_J && grid && s2w && xd, "ia_forward_skin: null pointer");
  IA_CHECK_ARG(grid->D > 0 && grid->H > 0 && grid->W > 0 && (long)grid->D * grid->H * grid->W * 48 < (1l << 32), "ia_forward_skin: bad grid");
  IA_CHECK_ARG((reinterpret_cast<uintptr_t>(voxel_J) & 15) == 0, "ia_forward_skin: the transform grid must be 16-byte aligned");
  hipLaunchKernelGGL(k_forward_skin, dim3(ia_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, xc, n, voxel_J, ia_make_grid_dev(grid), s2w, xd);
  IA_LAUNCH_CHECK("k_forward_skin");
  return IA_OK;
}
