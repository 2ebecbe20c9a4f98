// ia_meshops.hip -- processing of extracted meshes (no counterpart in the reference): vertex clustering with quadrics, Taubin
// smoothing, vertex normals from the faces.
//   cells of the vertices, rank of the occupied cells, kept faces and clusters, incidence lists   (ia_mesh_cluster_count)
//   faces, the vertex map, one 3 x 3 solve per kept cluster                                       (ia_mesh_cluster_emit)
//   per vertex: its valid faces and its distinct neighbours, ascending                            (ia_mesh_adjacency_build)
//   lambda / mu half-steps over the neighbour lists                                               (ia_mesh_taubin)
//   area-weighted face normals summed per vertex                                                  (ia_mesh_vertex_normals)
// The definitions are stated in DESIGN.md section 4 ("mesh simplification") and in include/instantavatar_hip_meshops.h.  Nothing
// here synchronises, allocates or reads on the host.
//
// All three operations need "for every key, its values in ascending order" (per cluster the face corners and the members, per
// vertex the faces and the neighbours).  seg_build makes it: count per key with integer atomics, exclusive scan, fill through a
// per-key cursor (any order), then every segment is sorted in place -- so what is read afterwards does not depend on the
// order the atomics were served in.  Every floating-point sum is then taken by ONE lane walking ONE sorted segment, in fp64.
// A vertex's lists are short (valence ~6): one lane sorts each.  A cell of 4^3 lattice cells holds a few hundred corners: one
// wave ranks such a segment in LDS.  The hub of a fan or a very coarse cell can pass the LDS buffer: that segment is sorted by
// one lane's in-place heapsort and, like every segment, summed by a single lane: slow, not wrong, no fixed-size per-thread array.
// The scan and the fill are ia_scan.h's; the face pieces and the grid of cells are ia_mesh_dev.h's.
#include "ia_common.h"
#include "ia_mesh_dev.h"
#include "ia_scan.h"
#include "../../include/instantavatar_hip_meshops.h"

#define IA_MO_THREADS IA_SCAN_THREADS
#define IA_MO_SORT_SHORT 16      // segments up to here: one lane each, insertion sort
#define IA_MO_SORT_LDS 2048      // segments up to here: one wave each, ranked in LDS (16 KB); beyond: one lane, heapsort

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// segments: for every key its values, ascending
// ---------------------------------------------------------------------------------------------------------------------
// start [nk + 1]; cnt [nk]: the cursor while filling, then the number of values of the key (of DISTINCT values after a unique
// pass, which leaves them at vals[start[key]] .. + cnt[key]); vals [total]
struct Seg { int32_t *start, *cnt, *vals; };

// an emitter E turns item i into (key, value) pairs: e(i, sink) calls sink(key, value).  Pass 1 counts, pass 2 stores.
struct SinkCount {
  int32_t *cnt;
  __device__ __forceinline__ void operator()(int key, int value) const { (void)value; atomicAdd(&cnt[key], 1); }
};
struct SinkFill {
  Seg S;
  __device__ __forceinline__ void operator()(int key, int value) const { S.vals[S.start[key] + atomicAdd(&S.cnt[key], 1)] = value; }
};
template <class E, class K>
__global__ __launch_bounds__(IA_MO_THREADS) void k_seg_emit(E e, int n_items, K sink) {
  const long long i = (long long)blockIdx.x * IA_MO_THREADS + threadIdx.x;
  if (i < n_items) e((int)i, sink);
}

__device__ __forceinline__ void mo_sift(int32_t *a, int root, int n) {
  int32_t top = a[root];
  while (true) {
    int child = 2 * root + 1;
    if (child >= n) break;
    int32_t c = a[child];
    if (child + 1 < n) {
      const int32_t c2 = a[child + 1];
      if (c2 > c) { c = c2; child++; }
    }
    if (c <= top) break;
    a[root] = c;
    root = child;
  }
  a[root] = top;
}
// in place, ascending, by one lane: insertion sort for the usual short segment, heapsort (no scratch at all) for a very long one
__device__ void mo_sort(int32_t *a, int n) {
  if (n <= IA_MO_SORT_SHORT) {
    for (int i = 1; i < n; i++) {
      const int32_t x = a[i];
      int j = i - 1;
      while (j >= 0 && a[j] > x) { a[j + 1] = a[j]; j--; }
      a[j + 1] = x;
    }
    return;
  }
  for (int r = n / 2 - 1; r >= 0; r--) mo_sift(a, r, n);
  for (int end = n - 1; end > 0; end--) {
    const int32_t t = a[0]; a[0] = a[end]; a[end] = t;
    mo_sift(a, 0, end);
  }
}
// sorted a[0 .. n) -> its distinct values in front, their number returned
__device__ int mo_unique(int32_t *a, int n) {
  int m = 1;
  int32_t last = a[0];
  for (int i = 1; i < n; i++) {
    const int32_t x = a[i];
    if (x != last) { a[m++] = x; last = x; }
  }
  return m;
}

// one lane per key: the segments of up to IA_MO_SORT_SHORT values (valence ~6: nearly all of a vertex's lists)
__global__ __launch_bounds__(IA_MO_THREADS) void k_seg_sort(Seg S, int nk, int unique) {
  const long long key = (long long)blockIdx.x * IA_MO_THREADS + threadIdx.x;
  if (key >= nk) return;
  const int n = S.cnt[key];
  if (n < 2 || n > IA_MO_SORT_SHORT) return;
  int32_t *a = S.vals + S.start[key];
  mo_sort(a, n);
  if (unique) S.cnt[key] = mo_unique(a, n);
}

// one wave (= one workgroup) per key: the longer segments.  Up to IA_MO_SORT_LDS values are ranked in LDS -- rank = the number
// of values that are smaller, or equal and earlier, so equal values come out adjacent -- and written back in order, with the
// distinct ones compacted by ballots for a unique pass; a segment beyond that is sorted in place by lane 0.
__global__ __launch_bounds__(64) void k_seg_sort_long(Seg S, int nk, int unique) {
  __shared__ int32_t s_in[IA_MO_SORT_LDS], s_out[IA_MO_SORT_LDS];
  const int key = blockIdx.x, lane = threadIdx.x;
  const int n = S.cnt[key];                                  // (uniform over the workgroup: so is every branch around a barrier)
  if (n <= IA_MO_SORT_SHORT) return;
  int32_t *a = S.vals + S.start[key];
  if (n > IA_MO_SORT_LDS) {
    if (lane == 0) {
      mo_sort(a, n);
      if (unique) S.cnt[key] = mo_unique(a, n);
    }
    return;
  }
  for (int i = lane; i < n; i += 64) s_in[i] = a[i];
  __syncthreads();
  for (int i = lane; i < n; i += 64) {
    const int32_t x = s_in[i];
    int r = 0;
    for (int j = 0; j < n; j++) {
      const int32_t y = s_in[j];
      r += (y < x || (y == x && j < i)) ? 1 : 0;
    }
    s_out[r] = x;
  }
  __syncthreads();
  if (!unique) {
    for (int i = lane; i < n; i += 64) a[i] = s_out[i];
    return;
  }
  int kept = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const bool keep = i < n && (i == 0 || s_out[i - 1] != s_out[i]);
    const unsigned long long m = __ballot(keep);
    if (keep) a[kept + __popcll(m & ((1ull << lane) - 1ull))] = s_out[i];
    kept += __popcll(m);
  }
  if (lane == 0) S.cnt[key] = kept;
}

// n_items >= 1, nk >= 1
template <class E>
void seg_build(const E &e, int n_items, int nk, Seg S, int32_t *bsum, bool unique, hipStream_t s) {
  const dim3 b(IA_MO_THREADS), gi(ia_div_up(n_items, IA_MO_THREADS));
  ia_fill_i32(S.cnt, nk, 0, s);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_seg_emit<E, SinkCount>), gi, b, 0, s, e, n_items, SinkCount{S.cnt});
  ia_scan(LoadInt{S.cnt}, nk, bsum, S.start, nullptr, s);
  ia_fill_i32(S.cnt, nk, 0, s);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_seg_emit<E, SinkFill>), gi, b, 0, s, e, n_items, SinkFill{S});
  hipLaunchKernelGGL(k_seg_sort, dim3(ia_div_up(nk, IA_MO_THREADS)), b, 0, s, S, nk, unique ? 1 : 0);
  hipLaunchKernelGGL(k_seg_sort_long, dim3(nk), dim3(64), 0, s, S, nk, unique ? 1 : 0);
}

// ---------------------------------------------------------------------------------------------------------------------
// faces and vertices
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool mo_finite3(const float *__restrict__ verts, int v) {
  return ia_finite3(verts[(size_t)v * 3], verts[(size_t)v * 3 + 1], verts[(size_t)v * 3 + 2]);
}

// the valid faces: indices in [0, nv), pairwise different, all three vertices finite (vok)
__device__ __forceinline__ bool mo_face(const int32_t *__restrict__ faces, int f, int nv, const uint8_t *__restrict__ vok, int v[3]) {
  ia_face_load(faces, f, v);
  if (!ia_face_in_range(v, nv) || !ia_face_distinct(v)) return false;
  return vok[v[0]] && vok[v[1]] && vok[v[2]];
}

// n = (p1 - p0) x (p2 - p0) in fp64; p0 is returned as well
__device__ __forceinline__ void mo_face_normal(const float *__restrict__ verts, const int v[3], double n[3], double p0[3]) {
  double p[3][3];
  ia_face_corners(verts, v, p);
  ia_face_cross(p, n);
  p0[0] = p[0][0]; p0[1] = p[0][1]; p0[2] = p[0][2];
}

__global__ __launch_bounds__(IA_MO_THREADS) void k_mo_vok(const float *__restrict__ verts, int nv, uint8_t *__restrict__ vok) {
  const long long v = (long long)blockIdx.x * IA_MO_THREADS + threadIdx.x;
  if (v < nv) vok[v] = mo_finite3(verts, (int)v) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// adjacency
// ---------------------------------------------------------------------------------------------------------------------
struct EmitFaceIncidence {      // face f -> (vertex, f) per corner
  const int32_t *faces; const uint8_t *vok; int nv;
  template <class K> __device__ __forceinline__ void operator()(int f, const K &sink) const {
    int v[3];
    if (!mo_face(faces, f, nv, vok, v)) return;
    sink(v[0], f); sink(v[1], f); sink(v[2], f);
  }
};
struct EmitFaceNeighbours {     // face f -> (vertex, each of the other two) per corner
  const int32_t *faces; const uint8_t *vok; int nv;
  template <class K> __device__ __forceinline__ void operator()(int f, const K &sink) const {
    int v[3];
    if (!mo_face(faces, f, nv, vok, v)) return;
    sink(v[0], v[1]); sink(v[0], v[2]);
    sink(v[1], v[2]); sink(v[1], v[0]);
    sink(v[2], v[0]); sink(v[2], v[1]);
  }
};

struct AdjWs { uint8_t *vok; Seg inc, nb; int32_t *bsum; float *tmp; size_t bytes; };
AdjWs adj_carve(void *ws, int nv, int nf) {
  WsCarver w(ws, 0);
  AdjWs o;
  const size_t v = (size_t)(nv > 0 ? nv : 1), f = (size_t)(nf > 0 ? nf : 1);
  o.vok = w.take<uint8_t>(v);
  o.inc.start = w.take<int32_t>(v + 1);
  o.inc.cnt = w.take<int32_t>(v);
  o.inc.vals = w.take<int32_t>(3 * f);
  o.nb.start = w.take<int32_t>(v + 1);
  o.nb.cnt = w.take<int32_t>(v);
  o.nb.vals = w.take<int32_t>(6 * f);
  o.bsum = w.take<int32_t>((size_t)ia_div_up((long long)v + 1, IA_MO_THREADS) + 1);
  o.tmp = w.take<float>(3 * v);
  o.bytes = w.off;
  return o;
}

// one half-step: dst = fp32(src + step (mean of the neighbours in src - src)); a vertex without neighbours keeps its bits
__global__ __launch_bounds__(IA_MO_THREADS) void k_taubin_half(const float *__restrict__ src, int nv, const int32_t *__restrict__ start,
                                                               const int32_t *__restrict__ cnt, const int32_t *__restrict__ vals,
                                                               double step, float *__restrict__ dst) {
  const long long v = (long long)blockIdx.x * IA_MO_THREADS + threadIdx.x;
  if (v >= nv) return;
  const int n = cnt[v];
  const uint32_t *sb = reinterpret_cast<const uint32_t *>(src);
  uint32_t *db = reinterpret_cast<uint32_t *>(dst);
  if (n == 0) {
#pragma unroll
    for (int d = 0; d < 3; d++) db[(size_t)v * 3 + d] = sb[(size_t)v * 3 + d];
    return;
  }
  const int32_t *nb = vals + start[v];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int t = 0; t < n; t++) {
    const size_t u = (size_t)nb[t] * 3;
    s0 += (double)src[u]; s1 += (double)src[u + 1]; s2 += (double)src[u + 2];
  }
  const double c = (double)n;
  const double x0 = (double)src[(size_t)v * 3], x1 = (double)src[(size_t)v * 3 + 1], x2 = (double)src[(size_t)v * 3 + 2];
  dst[(size_t)v * 3] = (float)(x0 + step * (s0 / c - x0));
  dst[(size_t)v * 3 + 1] = (float)(x1 + step * (s1 / c - x1));
  dst[(size_t)v * 3 + 2] = (float)(x2 + step * (s2 / c - x2));
}

__global__ __launch_bounds__(IA_MO_THREADS) void k_mo_copy_u32(const uint32_t *__restrict__ src, long long n, uint32_t *__restrict__ dst) {
  const long long i = (long long)blockIdx.x * IA_MO_THREADS + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

__global__ __launch_bounds__(IA_MO_THREADS) void k_vertex_normals(const float *__restrict__ verts, const int32_t *__restrict__ faces, int nv,
                                                                  const int32_t *__restrict__ start, const int32_t *__restrict__ cnt,
                                                                  const int32_t *__restrict__ vals, float *__restrict__ normals) {
  const long long v = (long long)blockIdx.x * IA_MO_THREADS + threadIdx.x;
  if (v >= nv) return;
  const int n = cnt[v];
  const int32_t *inc = vals + start[v];
  double s[3] = {0.0, 0.0, 0.0};
  for (int t = 0; t < n; t++) {
    const int f = inc[t];
    const int fv[3] = {faces[(size_t)f * 3], faces[(size_t)f * 3 + 1], faces[(size_t)f * 3 + 2]};   // valid: it was listed
    double c[3], p0[3];
    mo_face_normal(verts, fv, c, p0);
    if (!ia_finite3(c[0], c[1], c[2])) continue;
    s[0] += c[0]; s[1] += c[1]; s[2] += c[2];
  }
  const double len = ia_len3d(s);
  const bool ok = len > 0.0 && len < (double)INFINITY;
#pragma unroll
  for (int d = 0; d < 3; d++) normals[(size_t)v * 3 + d] = ok ? (float)(s[d] / len) : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------
// clustering
// ---------------------------------------------------------------------------------------------------------------------
// (the grid and the cell of a coordinate: IaGrid, ia_grid_cell)
__global__ __launch_bounds__(IA_MO_THREADS) void k_cl_cells(const float *__restrict__ verts, int nv, IaGrid G, uint8_t *__restrict__ vok,
                                                            int32_t *__restrict__ vclus, uint32_t *mask) {
  const long long v = (long long)blockIdx.x * IA_MO_THREADS + threadIdx.x;
  if (v >= nv) return;
  const bool ok = mo_finite3(verts, (int)v);
  vok[v] = ok ? 1 : 0;
  int32_t key = -1;
  if (ok) {
    const int i = ia_grid_cell(verts[(size_t)v * 3], G.lo[0], G.inv_h, G.n[0]);
    const int j = ia_grid_cell(verts[(size_t)v * 3 + 1], G.lo[1], G.inv_h, G.n[1]);
    const int k = ia_grid_cell(verts[(size_t)v * 3 + 2], G.lo[2], G.inv_h, G.n[2]);
    key = (int32_t)(((long long)i * G.n[1] + j) * G.n[2] + k);         // < 2^27
    atomicOr(&mask[key >> 5], 1u << (key & 31));
  }
  vclus[v] = key;
}

// key -> rank of the cell among the occupied cells
__global__ __launch_bounds__(IA_MO_THREADS) void k_cl_rank(int nv, const uint32_t *__restrict__ mask, const int32_t *__restrict__ wbase,
                                                           int32_t *__restrict__ vclus) {
  const long long v = (long long)blockIdx.x * IA_MO_THREADS + threadIdx.x;
  if (v >= nv) return;
  const int32_t key = vclus[v];
  if (key < 0) return;
  vclus[v] = wbase[key >> 5] + __popc(mask[key >> 5] & ((1u << (key & 31)) - 1u));
}

// a valid face with three different clusters is kept and marks them as used (every writer stores the same 1)
__global__ __launch_bounds__(IA_MO_THREADS) void k_cl_mark_faces(const int32_t *__restrict__ faces, int nf, int nv, const uint8_t *__restrict__ vok,
                                                                 const int32_t *__restrict__ vclus, int32_t *__restrict__ fkeep, int32_t *used) {
  const long long f = (long long)blockIdx.x * IA_MO_THREADS + threadIdx.x;
  if (f >= nf) return;
  int v[3];
  int keep = 0;
  if (mo_face(faces, (int)f, nv, vok, v)) {
    const int c0 = vclus[v[0]], c1 = vclus[v[1]], c2 = vclus[v[2]];
    if (c0 != c1 && c1 != c2 && c0 != c2) {
      keep = 1;
      used[c0] = 1; used[c1] = 1; used[c2] = 1;
    }
  }
  fkeep[f] = keep;
}

struct EmitClusterCorners {     // face f -> (cluster of the corner's vertex, 3 f + k) per corner
  const int32_t *faces; const uint8_t *vok; const int32_t *vclus; int nv;
  template <class K> __device__ __forceinline__ void operator()(int f, const K &sink) const {
    int v[3];
    if (!mo_face(faces, f, nv, vok, v)) return;
    sink(vclus[v[0]], 3 * f); sink(vclus[v[1]], 3 * f + 1); sink(vclus[v[2]], 3 * f + 2);
  }
};
struct EmitClusterMembers {     // vertex v -> (its cluster, v)
  const int32_t *vclus;
  template <class K> __device__ __forceinline__ void operator()(int v, const K &sink) const {
    const int c = vclus[v];
    if (c >= 0) sink(c, v);
  }
};

// the clusters are numbered 0 .. nc - 1 <= nv - 1 by ascending key; arrays over clusters have nv entries
struct ClWs {
  uint32_t *mask; int32_t *wbase; uint8_t *vok; int32_t *vclus, *used, *cbase, *fkeep, *fbase, *bsum; Seg corner, member;
  size_t bytes; long long words;
};
ClWs cl_carve(void *ws, int nv, int nf, long long cells) {
  WsCarver w(ws, 0);
  ClWs o;
  const size_t v = (size_t)(nv > 0 ? nv : 1), f = (size_t)(nf > 0 ? nf : 1);
  o.words = ((cells > 0 ? cells : 1) + 31) >> 5;
  o.mask = w.take<uint32_t>((size_t)o.words);
  o.wbase = w.take<int32_t>((size_t)o.words + 1);
  o.vok = w.take<uint8_t>(v);
  o.vclus = w.take<int32_t>(v);
  o.used = w.take<int32_t>(v);
  o.cbase = w.take<int32_t>(v + 1);
  o.fkeep = w.take<int32_t>(f);
  o.fbase = w.take<int32_t>(f + 1);
  const long long most = (long long)(v > f ? v : f) + 1 > o.words ? (long long)(v > f ? v : f) + 1 : o.words;
  o.bsum = w.take<int32_t>((size_t)ia_div_up(most, IA_MO_THREADS) + 1);
  o.corner.start = w.take<int32_t>(v + 1);
  o.corner.cnt = w.take<int32_t>(v);
  o.corner.vals = w.take<int32_t>(3 * f);
  o.member.start = w.take<int32_t>(v + 1);
  o.member.cnt = w.take<int32_t>(v);
  o.member.vals = w.take<int32_t>(v);
  o.bytes = w.off;
  return o;
}

__global__ __launch_bounds__(IA_MO_THREADS) void k_cl_emit_faces(const int32_t *__restrict__ faces, int nf, const int32_t *__restrict__ vclus,
                                                                 const int32_t *__restrict__ fkeep, const int32_t *__restrict__ fbase,
                                                                 const int32_t *__restrict__ cbase, int32_t *__restrict__ faces_out, int cap) {
  const long long f = (long long)blockIdx.x * IA_MO_THREADS + threadIdx.x;
  if (f >= nf || !fkeep[f]) return;
  const int k = fbase[f];
  if ((uint32_t)k >= (uint32_t)cap) return;
#pragma unroll
  for (int e = 0; e < 3; e++) faces_out[(size_t)k * 3 + e] = cbase[vclus[faces[(size_t)f * 3 + e]]];   // kept: its clusters are used
}

__global__ __launch_bounds__(IA_MO_THREADS) void k_cl_emit_map(int nv, const int32_t *__restrict__ vclus, const int32_t *__restrict__ used,
                                                               const int32_t *__restrict__ cbase, int32_t *__restrict__ vert_cluster) {
  const long long v = (long long)blockIdx.x * IA_MO_THREADS + threadIdx.x;
  if (v >= nv) return;
  const int c = vclus[v];
  vert_cluster[v] = c >= 0 && used[c] ? cbase[c] : -1;
}

// one lane = one cluster: the quadric over its corners, the mean over its members, the regularised solve
__global__ __launch_bounds__(IA_MO_THREADS) void k_cl_solve(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                            const float *__restrict__ colors, int nv, IaGrid G, double reg,
                                                            const int32_t *__restrict__ used, const int32_t *__restrict__ cbase, Seg corner,
                                                            Seg member, float *__restrict__ verts_out, float *__restrict__ colors_out, int cap) {
  const long long c = (long long)blockIdx.x * IA_MO_THREADS + threadIdx.x;
  if (c >= nv || !used[c]) return;
  const int out = cbase[c];
  if ((uint32_t)out >= (uint32_t)cap) return;
  const int nm = member.cnt[c];                              // >= 1: a used cluster has a vertex
  const int32_t *mem = member.vals + member.start[c];
  const double h = (double)G.h;
  double o[3];
  {
    const int v0 = mem[0];
#pragma unroll
    for (int d = 0; d < 3; d++)
      o[d] = (double)G.lo[d] + ((double)ia_grid_cell(verts[(size_t)v0 * 3 + d], G.lo[d], G.inv_h, G.n[d]) + 0.5) * h;
  }
  double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
  const int nc = corner.cnt[c];
  const int32_t *cor = corner.vals + corner.start[c];
  for (int t = 0; t < nc; t++) {
    const int f = cor[t] / 3;
    const int fv[3] = {faces[(size_t)f * 3], faces[(size_t)f * 3 + 1], faces[(size_t)f * 3 + 2]};
    double n[3], p0[3];
    mo_face_normal(verts, fv, n, p0);
    const double L = ia_len3d(n);
    if (!(L > 0.0 && L < (double)INFINITY)) continue;
    const double g0 = n[0] / L, g1 = n[1] / L, g2 = n[2] / L, a = L * 0.5;
    const double d = -(g0 * (p0[0] - o[0]) + g1 * (p0[1] - o[1]) + g2 * (p0[2] - o[2]));
    const double a0 = a * g0, a1 = a * g1, a2 = a * g2, ad = a * d;
    A00 += a0 * g0; A01 += a0 * g1; A02 += a0 * g2; A11 += a1 * g1; A12 += a1 * g2; A22 += a2 * g2;
    b0 += ad * g0; b1 += ad * g1; b2 += ad * g2;
  }
  double m0 = 0.0, m1 = 0.0, m2 = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0;
  for (int t = 0; t < nm; t++) {
    const size_t u = (size_t)mem[t] * 3;
    m0 += (double)verts[u] - o[0]; m1 += (double)verts[u + 1] - o[1]; m2 += (double)verts[u + 2] - o[2];
    if (colors) { c0 += (double)colors[u]; c1 += (double)colors[u + 1]; c2 += (double)colors[u + 2]; }
  }
  const double cnt = (double)nm;
  m0 /= cnt; m1 /= cnt; m2 /= cnt;
  double x0 = m0, x1 = m1, x2 = m2;
  const double w = reg * (A00 + A11 + A22);
  if (w > 0.0 && w < (double)INFINITY) {
    // (A + w I) x = w m - b by Cholesky: symmetric positive definite, condition number at most (1 + reg) / reg
    const double M00 = A00 + w, M11 = A11 + w, M22 = A22 + w;
    const double r0 = w * m0 - b0, r1 = w * m1 - b1, r2 = w * m2 - b2;
    const double l00 = sqrt(M00);
    const double l10 = A01 / l00, l20 = A02 / l00;
    const double l11 = sqrt(M11 - l10 * l10);
    const double l21 = (A12 - l20 * l10) / l11;
    const double l22 = sqrt(M22 - l20 * l20 - l21 * l21);
    const double y0 = r0 / l00;
    const double y1 = (r1 - l10 * y0) / l11;
    const double y2 = (r2 - l20 * y0 - l21 * y1) / l22;
    x2 = y2 / l22;
    x1 = (y1 - l21 * x2) / l11;
    x0 = (y0 - l10 * x1 - l20 * x2) / l00;
  }
  const double hh = h * 0.5;
  x0 = x0 < -hh ? -hh : (x0 > hh ? hh : x0);
  x1 = x1 < -hh ? -hh : (x1 > hh ? hh : x1);
  x2 = x2 < -hh ? -hh : (x2 > hh ? hh : x2);
  verts_out[(size_t)out * 3] = (float)(o[0] + x0);
  verts_out[(size_t)out * 3 + 1] = (float)(o[1] + x1);
  verts_out[(size_t)out * 3 + 2] = (float)(o[2] + x2);
  if (colors && colors_out) {
    colors_out[(size_t)out * 3] = (float)(c0 / cnt);
    colors_out[(size_t)out * 3 + 1] = (float)(c1 / cnt);
    colors_out[(size_t)out * 3 + 2] = (float)(c2 / cnt);
  }
}

// the sizes, the box and the cell edge, checked; the grid and its number of cells
static_assert(IA_CLUSTER_MAX_CELLS == 1ll << 27, "the text below");
int cl_check(const char *who, int nv, int nf, const float lo[3], const float hi[3], float h, float inv_h, IaGrid *G, long long *cells) {
  IA_CHECK_ARG(nv >= 0 && nf >= 0, "%s: negative size", who);
  IA_CHECK_ARG(nf <= IA_MESHOPS_MAX_FACES, "%s: nf = %d above %d, the most whose 6 nf neighbour entries an int32 offset reaches", who, nf,
               IA_MESHOPS_MAX_FACES);
  return ia_grid_check(who, lo, hi, h, inv_h, false, IA_CLUSTER_MAX_CELLS, "2^27", G, cells);
}

__global__ void k_mo_set2(int32_t *p, int32_t a, int32_t b) { p[0] = a; p[1] = b; }

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------
extern "C" size_t ia_mesh_adjacency_workspace_bytes(int nv, int nf) {
  if (nv < 0 || nf < 0 || nf > IA_MESHOPS_MAX_FACES) return 0;
  return adj_carve(nullptr, nv, nf).bytes;
}

extern "C" int ia_mesh_adjacency_build(const float *verts, const int32_t *faces, int nv, int nf, void *ws, size_t ws_bytes, void *stream) {
  IA_CHECK_ARG(nv >= 0 && nf >= 0, "ia_mesh_adjacency_build: negative size");
  IA_CHECK_ARG(nf <= IA_MESHOPS_MAX_FACES, "ia_mesh_adjacency_build: nf = %d above %d, the most whose 6 nf neighbour entries an int32 offset reaches",
               nf, IA_MESHOPS_MAX_FACES);
  IA_CHECK_ARG(ws && (nv == 0 || verts) && (nf == 0 || faces), "ia_mesh_adjacency_build: null pointer");
  const AdjWs W = adj_carve(ws, nv, nf);
  if (ws_bytes < W.bytes) return ia_set_error(IA_ERR_WORKSPACE, "ia_mesh_adjacency_build: workspace too small");
  if (nv == 0) return IA_OK;
  hipStream_t s = (hipStream_t)stream;
  if (nf == 0) {                 // no face: every list is empty
    ia_fill_i32(W.inc.cnt, nv, 0, s);
    ia_fill_i32(W.inc.start, (long long)nv + 1, 0, s);
    ia_fill_i32(W.nb.cnt, nv, 0, s);
    ia_fill_i32(W.nb.start, (long long)nv + 1, 0, s);
    IA_LAUNCH_CHECK("k_fill_i32");
    return IA_OK;
  }
  hipLaunchKernelGGL(k_mo_vok, dim3(ia_div_up(nv, IA_MO_THREADS)), dim3(IA_MO_THREADS), 0, s, verts, nv, W.vok);
  seg_build(EmitFaceIncidence{faces, W.vok, nv}, nf, nv, W.inc, W.bsum, false, s);
  seg_build(EmitFaceNeighbours{faces, W.vok, nv}, nf, nv, W.nb, W.bsum, true, s);
  IA_LAUNCH_CHECK("k_seg_sort");
  return IA_OK;
}

extern "C" int ia_mesh_taubin(const float *verts, int nv, int nf, void *ws, size_t ws_bytes, double lam, double mu, int iters, float *out,
                              void *stream) {
  IA_CHECK_ARG(nv >= 0 && nf >= 0 && nf <= IA_MESHOPS_MAX_FACES, "ia_mesh_taubin: bad size");
  IA_CHECK_ARG(iters >= 0, "ia_mesh_taubin: iters = %d < 0", iters);
  IA_CHECK_ARG(lam == lam && mu == mu, "ia_mesh_taubin: a step is NaN");
  if (nv == 0) return IA_OK;
  IA_CHECK_ARG(verts && out && ws, "ia_mesh_taubin: null pointer");
  IA_CHECK_ARG(verts != out, "ia_mesh_taubin: out aliases verts");
  const AdjWs W = adj_carve(ws, nv, nf);
  if (ws_bytes < W.bytes) return ia_set_error(IA_ERR_WORKSPACE, "ia_mesh_taubin: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const dim3 b(IA_MO_THREADS), g(ia_div_up(nv, IA_MO_THREADS));
  if (iters == 0)
    hipLaunchKernelGGL(k_mo_copy_u32, dim3(ia_div_up(3ll * nv, IA_MO_THREADS)), b, 0, s, reinterpret_cast<const uint32_t *>(verts), 3ll * nv,
                       reinterpret_cast<uint32_t *>(out));
  const float *src = verts;
  for (int it = 0; it < iters; it++) {
    hipLaunchKernelGGL(k_taubin_half, g, b, 0, s, src, nv, (const int32_t *)W.nb.start, (const int32_t *)W.nb.cnt, (const int32_t *)W.nb.vals, lam, W.tmp);
    hipLaunchKernelGGL(k_taubin_half, g, b, 0, s, (const float *)W.tmp, nv, (const int32_t *)W.nb.start, (const int32_t *)W.nb.cnt,
                       (const int32_t *)W.nb.vals, mu, out);
    src = out;
  }
  IA_LAUNCH_CHECK("k_taubin_half");
  return IA_OK;
}

extern "C" int ia_mesh_vertex_normals(const float *verts, const int32_t *faces, int nv, int nf, const void *ws, size_t ws_bytes,
                                      float *normals, void *stream) {
  IA_CHECK_ARG(nv >= 0 && nf >= 0 && nf <= IA_MESHOPS_MAX_FACES, "ia_mesh_vertex_normals: bad size");
  if (nv == 0) return IA_OK;
  IA_CHECK_ARG(verts && normals && ws && (nf == 0 || faces), "ia_mesh_vertex_normals: null pointer");
  const AdjWs W = adj_carve(const_cast<void *>(ws), nv, nf);
  if (ws_bytes < W.bytes) return ia_set_error(IA_ERR_WORKSPACE, "ia_mesh_vertex_normals: workspace too small");
  hipLaunchKernelGGL(k_vertex_normals, dim3(ia_div_up(nv, IA_MO_THREADS)), dim3(IA_MO_THREADS), 0, (hipStream_t)stream, verts, faces, nv,
                     (const int32_t *)W.inc.start, (const int32_t *)W.inc.cnt, (const int32_t *)W.inc.vals, normals);
  IA_LAUNCH_CHECK("k_vertex_normals");
  return IA_OK;
}

extern "C" size_t ia_mesh_cluster_workspace_bytes(int nv, int nf, long long n_cells) {
  if (nv < 0 || nf < 0 || nf > IA_MESHOPS_MAX_FACES || n_cells < 1 || n_cells > IA_CLUSTER_MAX_CELLS) return 0;
  return cl_carve(nullptr, nv, nf, n_cells).bytes;
}

extern "C" int ia_mesh_cluster_count(const float *verts, const int32_t *faces, int nv, int nf, float lo_x, float lo_y, float lo_z,
                                     float hi_x, float hi_y, float hi_z, float h, float inv_h, void *ws, size_t ws_bytes, int32_t *counts,
                                     void *stream) {
  const float lo[3] = {lo_x, lo_y, lo_z}, hi[3] = {hi_x, hi_y, hi_z};
  IaGrid G;
  long long cells;
  const int rc = cl_check("ia_mesh_cluster_count", nv, nf, lo, hi, h, inv_h, &G, &cells);
  if (rc) return rc;
  IA_CHECK_ARG(ws && counts && (nv == 0 || verts) && (nf == 0 || faces), "ia_mesh_cluster_count: null pointer");
  const ClWs W = cl_carve(ws, nv, nf, cells);
  if (ws_bytes < W.bytes) return ia_set_error(IA_ERR_WORKSPACE, "ia_mesh_cluster_count: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  if (nv == 0 || nf == 0) {      // no face is kept, so no cluster is
    hipLaunchKernelGGL(k_mo_set2, dim3(1), dim3(1), 0, s, counts, 0, 0);
    IA_LAUNCH_CHECK("k_mo_set2");
    return IA_OK;
  }
  const dim3 b(IA_MO_THREADS), gv(ia_div_up(nv, IA_MO_THREADS)), gf(ia_div_up(nf, IA_MO_THREADS));
  ia_fill_i32(reinterpret_cast<int32_t *>(W.mask), W.words, 0, s);
  ia_fill_i32(W.used, nv, 0, s);
  hipLaunchKernelGGL(k_cl_cells, gv, b, 0, s, verts, nv, G, W.vok, W.vclus, W.mask);
  ia_scan(LoadPopc{W.mask}, W.words, W.bsum, W.wbase, nullptr, s);
  hipLaunchKernelGGL(k_cl_rank, gv, b, 0, s, nv, (const uint32_t *)W.mask, (const int32_t *)W.wbase, W.vclus);
  hipLaunchKernelGGL(k_cl_mark_faces, gf, b, 0, s, faces, nf, nv, (const uint8_t *)W.vok, (const int32_t *)W.vclus, W.fkeep, W.used);
  ia_scan(LoadInt{W.fkeep}, nf, W.bsum, W.fbase, counts + 1, s);
  ia_scan(LoadInt{W.used}, nv, W.bsum, W.cbase, counts, s);
  seg_build(EmitClusterCorners{faces, W.vok, W.vclus, nv}, nf, nv, W.corner, W.bsum, false, s);
  seg_build(EmitClusterMembers{W.vclus}, nv, nv, W.member, W.bsum, false, s);
  IA_LAUNCH_CHECK("k_seg_sort");
  return IA_OK;
}

extern "C" int ia_mesh_cluster_emit(const float *verts, const int32_t *faces, const float *colors, int nv, int nf, float lo_x, float lo_y,
                                    float lo_z, float hi_x, float hi_y, float hi_z, float h, float inv_h, double reg, const void *ws,
                                    size_t ws_bytes, float *verts_out, int nv_out, int32_t *faces_out, int nf_out, float *colors_out,
                                    int32_t *vert_cluster, void *stream) {
  const float lo[3] = {lo_x, lo_y, lo_z}, hi[3] = {hi_x, hi_y, hi_z};
  IaGrid G;
  long long cells;
  const int rc = cl_check("ia_mesh_cluster_emit", nv, nf, lo, hi, h, inv_h, &G, &cells);
  if (rc) return rc;
  IA_CHECK_ARG(reg > 0.0 && reg < (double)INFINITY, "ia_mesh_cluster_emit: reg = %g must be positive and finite", reg);
  IA_CHECK_ARG(nv_out >= 0 && nf_out >= 0, "ia_mesh_cluster_emit: negative capacity");
  IA_CHECK_ARG(ws && (nv == 0 || verts) && (nf == 0 || faces) && (nv_out == 0 || verts_out) && (nf_out == 0 || faces_out),
               "ia_mesh_cluster_emit: null pointer");
  IA_CHECK_ARG((colors != nullptr) == (colors_out != nullptr) || nv_out == 0 || nv == 0, "ia_mesh_cluster_emit: colors and colors_out go together");
  const ClWs W = cl_carve(const_cast<void *>(ws), nv, nf, cells);
  if (ws_bytes < W.bytes) return ia_set_error(IA_ERR_WORKSPACE, "ia_mesh_cluster_emit: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  if (nv == 0) return IA_OK;
  if (nf == 0) {
    if (vert_cluster) ia_fill_i32(vert_cluster, nv, -1, s);
    IA_LAUNCH_CHECK("k_fill_i32");
    return IA_OK;
  }
  const dim3 b(IA_MO_THREADS), gv(ia_div_up(nv, IA_MO_THREADS)), gf(ia_div_up(nf, IA_MO_THREADS));
  if (vert_cluster)
    hipLaunchKernelGGL(k_cl_emit_map, gv, b, 0, s, nv, (const int32_t *)W.vclus, (const int32_t *)W.used, (const int32_t *)W.cbase, vert_cluster);
  if (nf_out > 0)
    hipLaunchKernelGGL(k_cl_emit_faces, gf, b, 0, s, faces, nf, (const int32_t *)W.vclus, (const int32_t *)W.fkeep, (const int32_t *)W.fbase,
                       (const int32_t *)W.cbase, faces_out, nf_out);
  if (nv_out > 0)
    hipLaunchKernelGGL(k_cl_solve, gv, b, 0, s, verts, faces, colors, nv, G, reg, (const int32_t *)W.used, (const int32_t *)W.cbase, W.corner,
                       W.member, verts_out, colors_out, nv_out);
  IA_LAUNCH_CHECK("k_cl_solve");
  return IA_OK;
}
