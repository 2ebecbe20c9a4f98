/*
 * instantavatar_hip_texture.h -- texture-atlas entry points of libinstantavatar_hip.so (csrc/ia_texture.hip): the per-face block
 * layout, the surface point of every texel, the snap of a texel onto the level set along the face normal, bilinear sampling of the
 * atlas.  Conventions as in instantavatar_hip.h (device pointers, `stream` as void*, no synchronisation, no allocation, 0 = IA_OK);
 * a header of its own, bound by `_lib` as a table of its own.  Definitions: DESIGN.md section 4, "texture atlas".
 *
 * Layout.  Block edge B texels, IA_TEX_MIN_BLOCK <= B <= IA_TEX_MAX_BLOCK, L = B - 3.  Face f lies in block q = f >> 1, half h = f & 1;
 * nb = max(1, ceil(sqrt(ceil(nf / 2)))) in integers, T = nb B <= IA_TEX_MAX_SIZE; block q has its origin at texel ((q % nb) B,
 * (q / nb) B).  Texel (i, j) of a block belongs to the half-0 face iff i + j <= B - 2, else to the half-1 face; a texel whose face
 * index is >= nf has owner -1.  Corners, in texels local to the block: half 0: (0, 0), (L, 0), (0, L); half 1: (B-1, B-1), (B-1-L, B-1),
 * (B-1, B-1-L).  Continuous texel coordinates put the centre of texel i at i + 0.5.
 */
#ifndef INSTANTAVATAR_HIP_TEXTURE_H
#define INSTANTAVATAR_HIP_TEXTURE_H

#include "instantavatar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IA_TEX_MIN_BLOCK 4
#define IA_TEX_MAX_BLOCK 64
#define IA_TEX_MAX_SIZE 16384
#define IA_TEX_MIN_STEPS 3
#define IA_TEX_MAX_STEPS 17

/* ia_tex_atlas_size (host only): T for nf >= 0 faces and block edge B; 0 when B or T lies outside the limits or nf < 0.
 * ia_tex_corner_uv: uv [nf,3,2] fp32 = the continuous texel coordinates (x, y) of the three corners of every face (exact in fp32).
 *   T must equal ia_tex_atlas_size(nf, B).                                                                                      */
int ia_tex_atlas_size(int nf, int B);
int ia_tex_corner_uv(int nf, int B, int T, float *uv, void *stream);

/* ia_tex_texel_points: the texels first .. first + count of the atlas in row-major order (texel g = y T + x).  For a texel owned by
 *   face f = (a, b, c) with local indices (i, j) (half 1: (B-1-i, B-1-j)): u1 = i / L, u2 = j / L, u0 = 1 - u1 - u2,
 *   p = u0 a + u1 b + u2 c (affine: the gutter diagonals with u0 < 0 are extrapolated), n = the unit normal (b - a) x (c - a), the
 *   zero vector when the product is zero or not finite -- all in fp64 on the fp32 vertices.
 *     pts [count,3]    = fp32(p + (t_scalar + t[i]) n)   (t [count] may be NULL: 0)
 *     normal [count,3] = fp32(n)                         (may be NULL)
 *     owner [count]    = f                               (may be NULL)
 *   A face with an index outside [0, nv) or a vertex with a non-finite coordinate owns nothing: its texels, like those of face
 *   indices >= nf, get owner -1 and zeros in pts and normal.                                                                   */
int ia_tex_texel_points(const float *verts, int nv, const int32_t *faces, int nf, int B, int T, int first, int count, const float *t,
                        float t_scalar, float *pts, float *normal, int32_t *owner, void *stream);

/* ia_tex_snap: sigma [K,n] fp32 = the density of n texels at the K offsets t_k = (k - (K-1)/2) h along the normal, h = 2 dist /
 *   (K-1) in fp32; K odd, IA_TEX_MIN_STEPS <= K <= IA_TEX_MAX_STEPS; dist >= 0 and finite.  s_k = sigma_k - level in fp32; interval
 *   k is a crossing when (s_k >= 0) != (s_k+1 >= 0) and both are finite, with the root t* = t_k + h (s_k / (s_k - s_k+1)) in fp32 in
 *   that order.  t_out [n] = the root with the smallest |t*| (a tie: the smaller k); 0 without a crossing, and the texel then counts
 *   into *unsnapped (device int32, ACCUMULATED: the caller zeroes it) when its owner is >= 0 (owner may be NULL: all owned).
 *   Texels with owner < 0 get 0 and are not counted.  dist == 0: t_out = 0 everywhere, nothing is counted.                   */
int ia_tex_snap(const float *sigma, int K, int n, float level, float dist, const int32_t *owner, float *t_out, int32_t *unsnapped,
                void *stream);

/* ia_tex_sample: rgb_out [R,3] = the atlas [T,T,3] fp32 filtered bilinearly at uv [R,2] (continuous texel coordinates x, y).  Per
 *   axis x = clamp(u - 0.5, 0, T-1), i0 = floor(x), i1 = min(i0 + 1, T-1), fx = x - i0; two lerps in x, then one in y, each as
 *   fma(w, b - a, a) in fp32.  A row with mask[r] == 0 (mask may be NULL) or a non-finite uv gives 0.                         */
int ia_tex_sample(const float *atlas, int T, const float *uv, const float *mask, int R, float *rgb_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_TEXTURE_H */
