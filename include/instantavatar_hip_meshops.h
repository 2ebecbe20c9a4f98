/*
 * instantavatar_hip_meshops.h -- mesh processing entry points of libinstantavatar_hip.so (csrc/ia_meshops.hip): vertex clustering
 * with quadrics, Taubin smoothing, vertex normals from the faces.  Conventions as in instantavatar_hip.h (device pointers, `stream`
 * as void*, no synchronisation, no allocation, scratch through `ws`, 0 = IA_OK); a header of its own, bound by `_lib` as a table of
 * its own.  Definitions: DESIGN.md section 4, "mesh simplification".
 *
 * Common to all of them.  A face is VALID when its three indices lie in [0, nv), are pairwise different and name vertices whose
 * three coordinates are finite; every other face is ignored, and a vertex with a non-finite coordinate takes part in nothing.
 * Arithmetic is fp64 on the fp32 inputs converted exactly, every sum runs in ascending order of what it sums over, integer
 * atomics only count: two calls on the same input give the same bytes.
 */
#ifndef INSTANTAVATAR_HIP_MESHOPS_H
#define INSTANTAVATAR_HIP_MESHOPS_H

#include "instantavatar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- vertex clustering on a uniform grid, one output vertex per occupied cell at the regularised minimiser of the cell's quadric.
 * Box [lo, hi] and cell edge h > 0 by value; inv_h = fp32(1 / h) formed by the caller.  Cells per axis n_a = max(1, ceil((hi_a -
 * lo_a) / h)) in fp64; n_cells = n_x n_y n_z <= IA_CLUSTER_MAX_CELLS and nf <= IA_MESHOPS_MAX_FACES, else an argument error.
 * Cell of a vertex, per axis: clamp((int)floorf((p_a - lo_a) * inv_h), 0, n_a - 1) in fp32; key = (i n_y + j) n_z + k.
 *   - cluster = the finite vertices of one cell; centre o = lo + (ijk + 1/2) h in fp64;
 *   - quadric: for every valid face f and corner k whose vertex lies in the cluster, by ascending 3 f + k: n = (p1 - p0) x (p2 - p0),
 *     L = |n| (skipped when 0 or not finite), nh = n / L, a = L / 2, d = -nh . (p0 - o); A += a nh nh^T, b += a d nh;
 *   - m = mean of the members' p - o, by ascending vertex index; w = reg trace(A); x solves (A + w I) x = w m - b when w > 0 and
 *     finite (Cholesky), else x = m; every component clamped to [-h/2, h/2]; output vertex = fp32(o + x);
 *   - a valid face whose three clusters differ is kept, in order, with its winding; duplicates stay; a cluster no kept face uses
 *     is dropped; the kept clusters are numbered by ascending key.
 * ia_mesh_cluster_count: counts (device, 2 x int32) = output vertices, output faces.  ws: ia_mesh_cluster_workspace_bytes(nv, nf,
 *   n_cells), read again by ia_mesh_cluster_emit (same verts, faces, box, h, inv_h).
 * ia_mesh_cluster_emit: verts_out [nv_out,3], faces_out [nf_out,3], colors_out [nv_out,3] = the fp64 mean of the members' colours
 *   by ascending vertex index (colors / colors_out may both be NULL), vert_cluster [nv] = the output vertex of every input vertex,
 *   -1 without one (may be NULL).  nv_out / nf_out: capacities in rows; rows past them are not written.                    */
#define IA_CLUSTER_MAX_CELLS 134217728ll
#define IA_MESHOPS_MAX_FACES 357913941
size_t ia_mesh_cluster_workspace_bytes(int nv, int nf, long long n_cells);
int ia_mesh_cluster_count(const float *verts, const int32_t *faces, int nv, int nf, float lo_x, float lo_y, float lo_z, float hi_x,
                          float hi_y, float hi_z, float h, float inv_h, void *ws, size_t ws_bytes, int32_t *counts, void *stream);
int ia_mesh_cluster_emit(const float *verts, const int32_t *faces, const float *colors, int nv, int nf, float lo_x, float lo_y,
                         float lo_z, float hi_x, float hi_y, float hi_z, float h, float inv_h, double reg, const void *ws,
                         size_t ws_bytes, float *verts_out, int nv_out, int32_t *faces_out, int nf_out, float *colors_out,
                         int32_t *vert_cluster, void *stream);

/* ---- per-vertex incidence of a mesh: for every vertex its valid faces in ascending order and its neighbours -- the distinct other
 * vertices of those faces -- in ascending order.  Built once into ws (ia_mesh_adjacency_workspace_bytes(nv, nf)), read by the two
 * calls below with the same nv, nf and faces.  nf <= IA_MESHOPS_MAX_FACES.
 * ia_mesh_taubin: out [nv,3] = `iters` iterations of x <- fp32(x + lam (mean_nb(x) - x)) followed by the same with mu, each
 *   half-step over all vertices from the previous half-step's buffer; the mean is the fp64 sum over the neighbours in ascending
 *   order over their number.  A vertex without neighbours keeps its bits; iters = 0 copies.  verts is not written; out must not
 *   alias it.  (ws also holds the buffer between the half-steps, hence not const.)
 * ia_mesh_vertex_normals: normals [nv,3] = the sum over the vertex's faces in ascending order of (p1 - p0) x (p2 - p0) in fp64 on
 *   `verts` (which may be other positions than the build saw; faces with a non-finite product are skipped), normalised in fp64;
 *   the zero vector where the sum is zero or not finite.                                                                     */
size_t ia_mesh_adjacency_workspace_bytes(int nv, int nf);
int ia_mesh_adjacency_build(const float *verts, const int32_t *faces, int nv, int nf, void *ws, size_t ws_bytes, void *stream);
int ia_mesh_taubin(const float *verts, int nv, int nf, void *ws, size_t ws_bytes, double lam, double mu, int iters, float *out,
                   void *stream);
int ia_mesh_vertex_normals(const float *verts, const int32_t *faces, int nv, int nf, const void *ws, size_t ws_bytes,
                           float *normals, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_MESHOPS_H */
