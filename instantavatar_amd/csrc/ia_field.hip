// ia_field.hip -- canonical field for gfx950: multiresolution hash-grid encoding
// fused with the sigma / colour tiny MLPs (MFMA 32x32x16 f16).
//
// Replaces NeRFNGPNet.forward (models/networks/ngp.py:73-83), i.e. tiny-cuda-nn
// v1.6 HashGrid + FullyFusedMLP(32-64-16) + FullyFusedMLP(16-64-64-16, sigmoid).
// Arithmetic contract (stated in DESIGN.md; the CPU checker restates it):
//   * table fp16; per level the 8 corner products are computed in fp32, rounded
//     to half and accumulated in half (tcnn kernel_grid);
//   * MLP: fp16 weights and activations, fp32 accumulation, activations rounded
//     to half between layers; sigma = half(out[0]); rgb = half(sigmoid(out)).
//
// Work decomposition (wave64):
//   * one lane = one sample during encoding; the level loop is wave-uniform, so
//     all 64 lanes gather from the SAME level table at the same time (coarse
//     levels: neighbouring samples share cache lines; level constants in SGPRs);
//   * the 32 features of a sample are the MFMA B operand (k = feature, n =
//     sample).  A 32x32x16 MFMA wants lane (n, h) to hold 8 consecutive k of
//     half h, so lanes j and j+32 exchange half of their features with
//     v_permlane32_swap: afterwards the wave holds two 32-sample column blocks;
//   * layer chaining needs no data movement: the C/D layout of one layer
//     (row = (r&3)+8(r>>2)+4h) is used directly as the B operand of the next,
//     the k-permutation is folded into the A (weight) fragments, which are
//     built once per workgroup in LDS (22 fragments x 64 lanes x 16 B).
#include "ia_common.h"
#include "ia_field_dev.h"

int ia_make_field_dev(const ia_field *f, FieldDev *o) {
  if (!f || !f->table || !f->sig_w1 || !f->sig_w2 || !f->col_w1 || !f->col_w2 || !f->col_w3) return -1;
  const int L = f->hash.n_levels;
  if (L != 8 && L != 16) return -2;
  for (int i = 0; i < 3; i++) { o->center[i] = f->center[i]; o->scale[i] = f->scale[i]; o->inv_unused[i] = 0; }
  o->lv.n_levels = L;
  for (int l = 0; l < IA_MAX_LEVELS; l++) {
    if (l < L) {
      const uint32_t size = f->hash.offset[l + 1] - f->hash.offset[l];
      const uint64_t r = f->hash.res[l];
      const bool dense = r * r * r <= (uint64_t)size;  // tcnn grid_index: hash iff size < stride
      if (!dense && (size & (size - 1)) != 0) return -3;  // hashed levels must be 2^k
      o->lv.scale[l] = f->hash.scale[l];
      o->lv.res[l] = f->hash.res[l];
      o->lv.offset[l] = f->hash.offset[l];
      o->lv.size[l] = size;
      o->lv.hashed[l] = dense ? 0u : 1u;
    } else {
      o->lv.scale[l] = 0; o->lv.res[l] = 1; o->lv.offset[l] = 0; o->lv.size[l] = 1; o->lv.hashed[l] = 0;
    }
  }
  o->table = reinterpret_cast<const uint32_t *>(f->table);
  o->sig_w1 = f->sig_w1; o->sig_w2 = f->sig_w2;
  o->col_w1 = f->col_w1; o->col_w2 = f->col_w2; o->col_w3 = f->col_w3;
  o->frags = f->mlp_frags;
  o->enc_ws = f->enc_ws;
  o->enc_ws_samples = f->enc_ws ? f->enc_ws_samples : 0;
  o->enc_split = (f->enc_split >= 1 && f->enc_split <= 3) ? f->enc_split : 2;
  // uniform-hash pattern (lets the kernel derive per-level pointers instead of holding 16 of them)
  uint32_t nd = 0;
  while ((int)nd < L && !o->lv.hashed[nd]) nd++;
  bool uni = (int)nd < L;
  for (int l = nd; l < L && uni; l++)
    uni = o->lv.hashed[l] && o->lv.size[l] == o->lv.size[nd] && o->lv.offset[l] == o->lv.offset[nd] + (l - nd) * o->lv.size[nd];
  o->n_dense = nd;
  o->hash_base = uni ? o->lv.offset[nd] : 0;
  o->hash_size = uni ? o->lv.size[nd] : 0;
  return 0;
}

// ---------------------------------------------------------------------------
// One level of the hash grid for one sample -> packed (f0,f1) half2.
//
// The cost of the encoding on gfx950 is the number of L1 (TCP) accesses: a 64-lane
// gather of 4-byte entries is served at ~1 lane per clock per CU, so the 16 x 8
// corner reads of a sample set the kernel's roofline.  Three access paths keep the
// reference arithmetic (same corner order, same half accumulation) while cutting
// the access count from 128 to ~80 per sample:
//   KIND 0  level table staged in LDS (the two coarsest dense levels, 70 KB);
//   KIND 1  dense level in global memory: the x-neighbours (cx, cx+1) are adjacent
//           entries -> ONE 8-byte load per corner pair;
//   KIND 2  hashed level: for even cx the pair differs only in index bit 0 -> one
//           aligned 8-byte load; odd cx adds a 4-byte load for the second corner.
// ---------------------------------------------------------------------------
struct __attribute__((packed, aligned(4))) U2A4 { uint32_t x, y; };

// Raw corner data of one level: v[8] (+ ext[4], meta for hashed levels), resolved later by
// level_reduce so that no load result is consumed inside the issue phase.
template <int KIND>
__device__ __forceinline__ void level_loads(const uint32_t *__restrict__ tab, float scale, uint32_t res,
                                            uint32_t size, const float xn[3], float w[3], uint32_t lo[4],
                                            uint32_t hi[4], uint32_t ext[4], uint32_t &meta) {
  uint32_t g[3];
  pos_fract(xn, scale, g, w);
  meta = 0;
  if (KIND == 2) {
    // hashed level (coherent prime hash, 2^k entries): eight independent 4-byte gathers.
    // (Merging the (cx, cx+1) pair of even cx into one aligned 8-byte slot saves 25 % of the
    // L1 accesses but needs a predicated second load; the register cost of deferring its
    // select spilled the 16-level kernel -- measured slower, see DESIGN.md.)
#pragma unroll
    for (int pr = 0; pr < 4; pr++) {
      const uint32_t cy = g[1] + (pr & 1), cz = g[2] + (pr >> 1);
      const uint32_t hsh = (cy * 2654435761u) ^ (cz * 805459861u);
      lo[pr] = tab[(g[0] ^ hsh) & (size - 1)];
      hi[pr] = tab[((g[0] + 1) ^ hsh) & (size - 1)];
      ext[pr] = 0u;
    }
    return;
  }
  const uint32_t tab0 = (KIND == 1) ? tab[0] : 0u;  // wave-uniform: entry 0 (wrap target of the last entry)
#pragma unroll
  for (int pr = 0; pr < 4; pr++) {  // corner pairs (cx, cx+1) at fixed (cy, cz): idx = 2*pr, 2*pr+1
    const uint32_t cy = g[1] + (pr & 1), cz = g[2] + (pr >> 1);
    uint32_t i0 = g[0] + cy * res + cz * res * res;  // < 2*size for clamped inputs (tcnn: index % size)
    if (i0 >= size) i0 -= size;
    i0 = min(i0, size - 1);  // memory safety for non-finite inputs
    ext[pr] = 0u;
    if (KIND == 0) {         // LDS-resident level
      uint32_t i1 = i0 + 1;
      if (i1 >= size) i1 -= size;
      lo[pr] = tab[i0];
      hi[pr] = tab[i1];
    } else {                 // dense level in global memory: ONE 8-byte load per x-neighbour pair
      const bool last = i0 == size - 1;  // only at the clamped border: i1 wraps to entry 0
      const U2A4 pair = *reinterpret_cast<const U2A4 *>(tab + (last ? size - 2 : i0));
      lo[pr] = pair.x;
      hi[pr] = pair.y;
      if (last) { meta |= 1u << pr; ext[pr] = tab0; meta |= 32u; }
    }
  }
}

template <int KIND>
__device__ __forceinline__ uint32_t level_reduce(const float w[3], const uint32_t lo[4], const uint32_t hi[4],
                                                 const uint32_t ext[4], uint32_t meta) {
  _Float16 r0 = (_Float16)0.f, r1 = (_Float16)0.f;
#pragma unroll
  for (int idx = 0; idx < 8; idx++) {
    float wt = 1.f;
    wt *= (idx & 1) ? w[0] : 1.f - w[0];
    wt *= (idx & 2) ? w[1] : 1.f - w[1];
    wt *= (idx & 4) ? w[2] : 1.f - w[2];
    const int pr = idx >> 1;
    uint32_t raw;
    if (KIND != 1) {
      raw = (idx & 1) ? hi[pr] : lo[pr];
    } else {
      // (lo/hi are separate arrays on purpose: `sel ? a[1] : a[0]` would be turned into a
      // dynamically indexed -- i.e. scratch -- access)
      const bool sel = (meta >> pr) & 1u;  // dense: pair wrapped around the end of the level
      const uint32_t c0 = sel ? hi[pr] : lo[pr];
      const uint32_t c1 = sel ? ext[pr] : hi[pr];
      raw = (idx & 1) ? c1 : c0;
    }
    union { uint32_t u; half2v h; } c;
    c.u = raw;
    r0 = r0 + (_Float16)(wt * (float)c.h.x);
    r1 = r1 + (_Float16)(wt * (float)c.h.y);
  }
  union { uint32_t u; half2v h; } o;
  o.h.x = r0; o.h.y = r1;
  return o.u;
}

// Encodes levels [L0, L0+N) of one sample.  All corner loads of the group are issued
// before the first use (straight-line code, no data-dependent control flow), so the
// group's gathers overlap.  NLDS: leading levels resident in LDS; NDENSE: number of
// dense (non-hashed) levels; NDENSE < 0: decide per level at run time (generic tables).
template <int L0, int N, int NLDS, int NDENSE>
__device__ __forceinline__ void encode_group(const FieldDev &F, const uint32_t *__restrict__ lds_tab,
                                             const float xn[3], uint32_t *__restrict__ feat) {
  float w[N][3];
  uint32_t lo[N][4], hi[N][4], ext[N][4], meta[N];
#pragma unroll
  for (int k = 0; k < N; k++) {
    const int l = L0 + k;
    const uint32_t *gt = F.table + F.lv.offset[(NDENSE >= 0 && l >= NDENSE) ? 0 : l];
    if (l < NLDS) level_loads<0>(lds_tab + F.lv.offset[l], F.lv.scale[l], F.lv.res[l], F.lv.size[l], xn, w[k], lo[k], hi[k], ext[k], meta[k]);
    else if (NDENSE >= 0 ? (l < NDENSE) : !F.lv.hashed[l]) level_loads<1>(gt, F.lv.scale[l], F.lv.res[l], F.lv.size[l], xn, w[k], lo[k], hi[k], ext[k], meta[k]);
    else if (NDENSE >= 0)  // uniform hashed levels: pointer and size derived, not stored per level
      level_loads<2>(F.table + F.hash_base + (uint32_t)(l - NDENSE) * F.hash_size, F.lv.scale[l], 0u, F.hash_size, xn,
                     w[k], lo[k], hi[k], ext[k], meta[k]);
    else level_loads<2>(gt, F.lv.scale[l], F.lv.res[l], F.lv.size[l], xn, w[k], lo[k], hi[k], ext[k], meta[k]);
  }
#pragma unroll
  for (int k = 0; k < N; k++) {
    const int l = L0 + k;
    if (l < NLDS) feat[l] = level_reduce<0>(w[k], lo[k], hi[k], ext[k], meta[k]);
    else if (NDENSE >= 0 ? (l < NDENSE) : !F.lv.hashed[l]) feat[l] = level_reduce<1>(w[k], lo[k], hi[k], ext[k], meta[k]);
    else feat[l] = level_reduce<2>(w[k], lo[k], hi[k], ext[k], meta[k]);
  }
}

template <int L, int NLDS, int NDENSE>
__device__ __forceinline__ void encode_all(const FieldDev &F, const uint32_t *__restrict__ lds_tab,
                                           const float xn[3], uint32_t *__restrict__ feat) {
  // groups of IA_ENC_GROUP levels: all gathers of a group are in flight together; the group
  // size is bounded by the register file (each level holds 12 raw words until it is reduced).
  // sched_barrier keeps the compiler from hoisting the next group's loads above this group's
  // reduction (which would spill).
#ifndef IA_ENC_GROUP
#define IA_ENC_GROUP 8
#endif
#pragma unroll
  for (int g0 = 0; g0 < L; g0 += IA_ENC_GROUP) {
    switch (g0) {  // compile-time after unrolling
      case 0: encode_group<0, IA_ENC_GROUP, NLDS, NDENSE>(F, lds_tab, xn, feat); break;
      case 2: encode_group<2, IA_ENC_GROUP, NLDS, NDENSE>(F, lds_tab, xn, feat); break;
      case 4: encode_group<4, IA_ENC_GROUP, NLDS, NDENSE>(F, lds_tab, xn, feat); break;
      case 6: encode_group<6, IA_ENC_GROUP, NLDS, NDENSE>(F, lds_tab, xn, feat); break;
      case 8: encode_group<(L > 8 ? 8 : 0), IA_ENC_GROUP, NLDS, NDENSE>(F, lds_tab, xn, feat); break;
      case 10: encode_group<(L > 8 ? 10 : 0), IA_ENC_GROUP, NLDS, NDENSE>(F, lds_tab, xn, feat); break;
      case 12: encode_group<(L > 8 ? 12 : 0), IA_ENC_GROUP, NLDS, NDENSE>(F, lds_tab, xn, feat); break;
      case 14: encode_group<(L > 8 ? 14 : 0), IA_ENC_GROUP, NLDS, NDENSE>(F, lds_tab, xn, feat); break;
    }
    asm volatile("" ::: "memory");  // loads of the next group stay below this group's reduction
    __builtin_amdgcn_sched_barrier(0);
  }
}


// ---------------------------------------------------------------------------
// XCD-sharded encoding.  The fp16 table (26 MB) does not fit one XCD's 4 MB L2, so
// when every workgroup walks all 16 levels each L2 thrashes and the hashed gathers
// are served across the fabric.  Here a workgroup encodes ONE hashed level (plus, in
// the second phase, one dense level) for a tile of samples, and the level is chosen
// from blockIdx % 8 -- the XCD the dispatcher places the workgroup on (observed
// placement; only speed depends on it).  Each XCD then gathers from a 2 MB slice
// that stays resident in its own L2:
//   phase A  (blocks s <  tiles):  XCD x -> hashed level ND+x          , tile s
//   phase B  (blocks s >= tiles):  XCD x -> hashed level ND+8+(x&3)    , tiles of
//            parity x>>2, together with dense level (x&3)
// (8-level tables have 4 hashed levels: phase B only).  Features are written as
// level-major planes [L][stride] of packed half2 (coalesced 256 B per wave) and
// consumed by k_field<..., PLANES>.  Per-level arithmetic is identical to
// level_loads/level_reduce, so the features are bit-identical.
// Hashed levels gather the aligned 16-byte group of four entries around corner x: the
// x-neighbour (x + 1) ^ h lies in the same group unless x mod 4 == 3 -> one 16-byte load
// per (y, z) pair; one lane in four adds a predicated 4-byte load (hashed_quad_loads).
// ---------------------------------------------------------------------------
#ifndef IA_ENC_S
#define IA_ENC_S 3  // samples per thread (table gathers in flight per lane: 4-5 per sample): training forward, ia_hashgrid_fwd_planes
#endif
// Samples per thread of the inference planes route (ia_launch_field without an activation record on the sharded path: the
// render loop, the occupancy probes, ia_deform_query).  The register footprint follows it -- 3: 124 VGPRs (128 allocated, 4
// waves per SIMD), 2: 86 (88, 5), 1: 51 (56, 8) -- and with it when a workgroup gets onto a CU beside other frames'
// k_search workgroups.  Measured (profiles/encode_coresidency_ab.txt): 2 is the fastest with three
// frames in flight and with one; 1 pays more for the fewer gathers in flight per wave than the residency returns.
// Per-sample arithmetic does not depend on the shape: features are bit-identical.
#ifndef IA_ENC_S_RENDER
#define IA_ENC_S_RENDER 2
#endif
#if IA_ENC_S < 1 || IA_ENC_S > 3 || IA_ENC_S_RENDER < 1 || IA_ENC_S_RENDER > 3
#error "IA_ENC_S and IA_ENC_S_RENDER must be 1, 2 or 3"
#endif
#define IA_ENC_THREADS 256
// Register budget of a shape: VGPRs allocated per wave (the compiler's count rounded up to the granule of 8) and the waves
// per SIMD that leaves of the 512-entry file (at most 8).  The budget is pinned with the second __launch_bounds__ argument;
// a workgroup is one wave per SIMD, so an XCD (32 CUs) holds 32 x enc_waves_per_simd(S) workgroups: the grid cap.
__host__ __device__ constexpr int enc_vgprs(int S) { return S == 1 ? 56 : S == 2 ? 88 : 128; }
__host__ __device__ constexpr int enc_waves_per_simd(int S) { return 512 / enc_vgprs(S) < 8 ? 512 / enc_vgprs(S) : 8; }
__host__ __device__ constexpr int enc_max_wg_per_xcd(int S) { return 32 * enc_waves_per_simd(S); }
// second __launch_bounds__ argument.  3 samples per thread stay unpinned (0): the budget of 128 is what the compiler takes
// by itself, and pinning it renames registers in code that is otherwise instruction for instruction the same.
__host__ __device__ constexpr int enc_pinned_waves(int S) { return S == 3 ? 0 : enc_waves_per_simd(S); }

// Round 6: the aligned 16-byte GROUP of four table entries around corner x instead of its aligned pair.  With tcnn's
// hash the x-neighbour of a corner is entry (x + 1) ^ h: inside the same aligned pair when x is even, inside the same aligned group
// of four unless x mod 4 == 3.  One dwordx4 gather per (y, z) pair then serves both x-corners for 3 lanes in 4 (the pair version: 2
// in 4), and the second, separate gather of the others touches a quarter instead of half of the wave's lanes: 4 x 64 + 4 x 16 = 320
// line look-ups per wave and level instead of 4 x 64 + 4 x 32 = 384 -- the vector L1's look-up rate is what bounds this kernel.
// Measured (profiles/r06_ab_encode_quad.txt): 2^20 random points 342 -> 325 us, a frame's samples 204 -> 190 us,
// features bit-identical; 578 -> 587-589 frames/s.  Three samples per thread (122 VGPRs, four waves per SIMD) instead of four with the
// wider records (160 VGPRs otherwise).  The pair version and its cache policies: tools/variants/encode_pair_r06.diff.txt,
// tools/variants/encode_cache_policy_r06.diff.txt.
__device__ __forceinline__ uint32_t quad_select(uint32_t x, uint32_t y, uint32_t z, uint32_t w, uint32_t s) {
  const uint32_t lo = (s & 1u) ? y : x, hi = (s & 1u) ? w : z;
  return (s & 2u) ? hi : lo;
}
__device__ __forceinline__ void hashed_quad_loads(const uint32_t *__restrict__ tab, float scale, uint32_t mask, const float xn[3],
                                                  float w[3], uint32_t qx[4], uint32_t qy[4], uint32_t qz[4], uint32_t qw[4],
                                                  uint32_t ext[4], uint32_t &meta) {
  uint32_t g[3];
  pos_fract(xn, scale, g, w);
  const bool far = (g[0] & 3u) == 3u;   // x + 1 carries out of the two low bits: its entry lies in another group
  meta = far ? (1u << 16) : 0u;
#pragma unroll
  for (int pr = 0; pr < 4; pr++) {
    const uint32_t cy = g[1] + (pr & 1), cz = g[2] + (pr >> 1);
    const uint32_t hsh = (cy * 2654435761u) ^ (cz * 805459861u);
    const uint32_t i0 = (g[0] ^ hsh) & mask, i1 = ((g[0] + 1) ^ hsh) & mask;
    const uint4 v = *reinterpret_cast<const uint4 *>(tab + (i0 & ~3u));
    qx[pr] = v.x; qy[pr] = v.y; qz[pr] = v.z; qw[pr] = v.w;
    meta |= ((i0 & 3u) | ((i1 & 3u) << 2)) << (4 * pr);
    ext[pr] = 0u;
    if (far) ext[pr] = tab[i1];
  }
}
__device__ __forceinline__ uint32_t hashed_quad_reduce(const float w[3], const uint32_t qx[4], const uint32_t qy[4], const uint32_t qz[4],
                                                       const uint32_t qw[4], const uint32_t ext[4], uint32_t meta) {
  _Float16 r0 = (_Float16)0.f, r1 = (_Float16)0.f;
  const bool far = meta & (1u << 16);
#pragma unroll
  for (int idx = 0; idx < 8; idx++) {   // the same eight weighted fp16 accumulations, in the same order, as level_reduce
    float wt = 1.f;
    wt *= (idx & 1) ? w[0] : 1.f - w[0];
    wt *= (idx & 2) ? w[1] : 1.f - w[1];
    wt *= (idx & 4) ? w[2] : 1.f - w[2];
    const int pr = idx >> 1;
    const uint32_t sel = (meta >> (4 * pr)) & 15u;
    const uint32_t c0 = quad_select(qx[pr], qy[pr], qz[pr], qw[pr], sel & 3u);
    const uint32_t c1 = far ? ext[pr] : quad_select(qx[pr], qy[pr], qz[pr], qw[pr], sel >> 2);
    union { uint32_t u; half2v h; } c;
    c.u = (idx & 1) ? c1 : c0;
    r0 = r0 + (_Float16)(wt * (float)c.h.x);
    r1 = r1 + (_Float16)(wt * (float)c.h.y);
  }
  union { uint32_t u; half2v h; } o;
  o.h.x = r0; o.h.y = r1;
  return o.u;
}

template <int L, int S>
__global__ __launch_bounds__(IA_ENC_THREADS, enc_pinned_waves(S)) void k_encode_xcd(const float *__restrict__ x, int V,
                                                                const int32_t *__restrict__ n_dev, FieldDev F,
                                                                uint32_t *__restrict__ planes, size_t stride) {
  constexpr int ND = 4, NH = L - ND;  // tcnn default pattern (checked by the host)
  constexpr int TILE = S * IA_ENC_THREADS;
  if (n_dev) V = min(V, *n_dev);
  const int n_tiles = (V + TILE - 1) / TILE;
  // Work items of an XCD: (16 levels) first EVERY tile of hashed level 4 + xcd, then tiles of the second level group -- hashed level
  // 12 + (xcd & 3) together with dense level (xcd & 3) -- which XCD k shares with XCD k + 4: of every four tiles XCD k takes the
  // first `spl`, XCD k + 4 the rest.  spl = F.enc_split is the caller's hint (ia_field.enc_split): on spatially coherent samples
  // (a frame's ray-ordered candidates, Morton-ordered probes) hashed levels 4-7 are much cheaper than 8-11 -- coarse cells, the
  // lanes of a wave share lines -- so XCDs 0-3 are given three tiles of four; on incoherent samples every level costs the same
  // and two of four is right (profiles/r06_ab_encode_quad.txt: 605 -> 612 frames/s with 3; random points 326 -> 393 us with 3).
  const int spl = NH > 4 ? F.enc_split : 2, sph = 4 - spl, mx = spl > sph ? spl : sph;
  const int n_items = (NH > 4 ? n_tiles : 0) + ((n_tiles + 3) >> 2) * mx;  // per XCD
  const int xcd = blockIdx.x & 7;
  for (int s = blockIdx.x >> 3; s < n_items; s += gridDim.x >> 3) {
    int tile, lev_h, lev_d;
    if (NH > 4 && s < n_tiles) {
      tile = s; lev_h = ND + xcd; lev_d = -1;
    } else {
      const int sb = NH > 4 ? s - n_tiles : s;
      const int q = sb / mx, r = sb - q * mx;
      if (r >= (xcd < 4 ? spl : sph)) continue;
      tile = q * 4 + (xcd < 4 ? r : spl + r); lev_h = (NH > 4 ? ND + 8 : ND) + (xcd & 3); lev_d = xcd & 3;
    }
    if (tile >= n_tiles) continue;
    const int base = tile * TILE + threadIdx.x;
    float xn[S][3];
#pragma unroll
    for (int k = 0; k < S; k++) {
      const int i = base + k * IA_ENC_THREADS;
      xn[k][0] = xn[k][1] = xn[k][2] = 0.f;
      if (i < V) normalise(F, x, (size_t)i, xn[k]);
    }
    {
      const uint32_t *tab = F.table + F.hash_base + (uint32_t)(lev_h - ND) * F.hash_size;
      const float scale = F.lv.scale[lev_h];
      float w[S][3];
      uint32_t *out = planes + (size_t)lev_h * stride;
      uint32_t qx[S][4], qy[S][4], qz[S][4], qw[S][4], ext[S][4], meta[S];
#pragma unroll
      for (int k = 0; k < S; k++) hashed_quad_loads(tab, scale, F.hash_size - 1, xn[k], w[k], qx[k], qy[k], qz[k], qw[k], ext[k], meta[k]);
#pragma unroll
      for (int k = 0; k < S; k++) {
        const int i = base + k * IA_ENC_THREADS;
        const uint32_t f = hashed_quad_reduce(w[k], qx[k], qy[k], qz[k], qw[k], ext[k], meta[k]);
        if (i < V) out[i] = f;
      }
    }
    if (lev_d >= 0) {
      const uint32_t *tab = F.table + F.lv.offset[lev_d];
      const float scale = F.lv.scale[lev_d];
      const uint32_t res = F.lv.res[lev_d], size = F.lv.size[lev_d];
      float w[S][3];
      uint32_t lo[S][4], hi[S][4], ext[S][4], meta[S];
#pragma unroll
      for (int k = 0; k < S; k++) level_loads<1>(tab, scale, res, size, xn[k], w[k], lo[k], hi[k], ext[k], meta[k]);
      uint32_t *out = planes + (size_t)lev_d * stride;
#pragma unroll
      for (int k = 0; k < S; k++) {
        const int i = base + k * IA_ENC_THREADS;
        const uint32_t f = level_reduce<1>(w[k], lo[k], hi[k], ext[k], meta[k]);
        if (i < V) out[i] = f;
      }
    }
  }
}

static inline bool ia_field_shardable(const FieldDev &F) {
  const int L = F.lv.n_levels;
  return (L == 8 || L == 16) && F.n_dense == 4 && F.hash_size != 0 && (F.hash_size & (F.hash_size - 1)) == 0;
}

template <int S>
static int ia_launch_encode_xcd_shape(const float *x, int V, const int32_t *n_dev, const FieldDev &F, uint32_t *planes,
                                      size_t stride, hipStream_t s) {
  constexpr int TILE = S * IA_ENC_THREADS;
  const int tiles = (V + TILE - 1) / TILE;
  const int L = F.lv.n_levels;
  const int spl = L == 16 ? F.enc_split : 2, mx = spl > 4 - spl ? spl : 4 - spl;
  int per_xcd = (L == 16 ? tiles : 0) + ((tiles + 3) / 4) * mx;
  if (per_xcd > enc_max_wg_per_xcd(S)) per_xcd = enc_max_wg_per_xcd(S);  // workgroups loop over their XCD's items
  if (L == 16)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_encode_xcd<16, S>), dim3(8 * per_xcd), dim3(IA_ENC_THREADS), 0, s, x, V, n_dev, F, planes, stride);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_encode_xcd<8, S>), dim3(8 * per_xcd), dim3(IA_ENC_THREADS), 0, s, x, V, n_dev, F, planes, stride);
  IA_LAUNCH_CHECK("k_encode_xcd");
  return IA_OK;
}

// `shape`: samples per thread, IA_ENC_S_RENDER (inference planes route) or IA_ENC_S (training forward, stand-alone planes)
static int ia_launch_encode_xcd(const float *x, int V, const int32_t *n_dev, const FieldDev &F, uint32_t *planes,
                                size_t stride, hipStream_t s, int shape) {
  if (shape == IA_ENC_S_RENDER) return ia_launch_encode_xcd_shape<IA_ENC_S_RENDER>(x, V, n_dev, F, planes, stride, s);
  if (shape == IA_ENC_S) return ia_launch_encode_xcd_shape<IA_ENC_S>(x, V, n_dev, F, planes, stride, s);
  return ia_set_error(IA_ERR_ARG, "ia_launch_encode_xcd: no instantiation for %d samples per thread", shape);
}

// activation record written in training mode (fp16, IA_ACT_STRIDE halves per sample):
//   [0,2L) hash features | h1 (64) | sigma-net output (16) | c1 (64) | c2 (64)
template <int G8>
__device__ __forceinline__ void save_rows(uint16_t *__restrict__ dst, const floatx16 &acc, int h, bool relu) {
  // C/D rows (r&3)+8(r>>2)+4h: four consecutive rows per register group -> one 8-byte store
#pragma unroll
  for (int g = 0; g < G8; g++) {
    union { _Float16 hh[4]; uint2 u; } c;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      float v = acc[4 * g + q];
      if (relu) v = v < 0.f ? 0.f : v;
      c.hh[q] = (_Float16)v;
    }
    *reinterpret_cast<uint2 *>(dst + 8 * g + 4 * h) = c.u;
  }
}

#ifndef IA_FIELD_THREADS
#define IA_FIELD_THREADS 768
#endif
// The planes-route inference instantiations (SAVE = false, PLANES = true: the render MLP behind k_encode_xcd) run as
// workgroups of one wave per SIMD, IA_FIELD_PLANES_WG_PER_CU of them per CU: the same 12 waves per CU and the same register
// budget per wave (IA_FIELD_PLANES_WAVES_PER_SIMD) as one 768-thread workgroup, but a workgroup needs 160 VGPRs per SIMD and
// 22 KB of LDS instead of 480 and a drained CU, so it starts beside three resident k_search workgroups.
// Training and the fused routes (up to 72 KB of staged table per workgroup) keep IA_FIELD_THREADS.
#ifndef IA_FIELD_PLANES_THREADS
#define IA_FIELD_PLANES_THREADS 256
#endif
#ifndef IA_FIELD_PLANES_WG_PER_CU
#define IA_FIELD_PLANES_WG_PER_CU 3
#endif
#ifndef IA_FIELD_PLANES_WAVES_PER_SIMD
#define IA_FIELD_PLANES_WAVES_PER_SIMD 3
#endif
__host__ __device__ constexpr int field_threads(bool save, bool planes) {
  return (planes && !save) ? IA_FIELD_PLANES_THREADS : IA_FIELD_THREADS;
}
__host__ __device__ constexpr int field_waves_per_simd(bool save, bool planes) {
  return (planes && !save) ? IA_FIELD_PLANES_WAVES_PER_SIMD : IA_FIELD_THREADS / 256;
}

template <int L, bool SAVE, int NLDS, int NDENSE, bool PLANES = false>
__global__ __launch_bounds__(field_threads(SAVE, PLANES), field_waves_per_simd(SAVE, PLANES)) void k_field(const float *__restrict__ x, int V,
                                               const int32_t *__restrict__ n_dev, FieldDev F,
                                               float *__restrict__ rgb, float *__restrict__ sigma,
                                               unsigned long long *prof, uint16_t *__restrict__ acts,
                                               int lds_entries, const uint32_t *__restrict__ planes = nullptr,
                                               size_t plane_stride = 0) {
  constexpr int ACT_STRIDE = 2 * L + 64 + 16 + 64 + 64;
  constexpr int THREADS = field_threads(SAVE, PLANES), WAVES = THREADS / 64;
  extern __shared__ __attribute__((aligned(16))) char s_dyn[];
  half8 (*s_frag)[64] = reinterpret_cast<half8 (*)[64]>(s_dyn);
  const uint32_t *s_tab = reinterpret_cast<const uint32_t *>(s_dyn + N_FRAG * 64 * 16);
  if (n_dev) V = min(V, *n_dev);
  if (prof && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(prof, (unsigned long long)V);
  const int n_tiles = (V + 63) >> 6;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // tiles go round-robin over workgroups first (consecutive workgroups land on different CUs), then over a
  // workgroup's waves: a small launch still spreads over all 256 CUs
  const int tile_stride = gridDim.x * WAVES;
  int tile = blockIdx.x + wave * gridDim.x;
  if ((int)blockIdx.x >= n_tiles) return;  // whole workgroup idle
  // stage the coarsest dense levels (entries [0, lds_entries) of the table) in LDS
  {
    uint32_t *dst = reinterpret_cast<uint32_t *>(s_dyn + N_FRAG * 64 * 16);
    const uint4 *src4 = reinterpret_cast<const uint4 *>(F.table);
    uint4 *dst4 = reinterpret_cast<uint4 *>(dst);
    for (int e = threadIdx.x; e < lds_entries / 4; e += THREADS) dst4[e] = src4[e];
  }
  // A fragments: copy the prebuilt image (ia_field_prepare) or build it here
  if (F.frags) {
    const uint4 *src = reinterpret_cast<const uint4 *>(F.frags);
    uint4 *dst = reinterpret_cast<uint4 *>(&s_frag[0][0]);
#pragma unroll
    for (int e = threadIdx.x; e < N_FRAG * 64; e += THREADS) dst[e] = src[e];
  } else {
    for (int e = threadIdx.x; e < N_FRAG * 64 * 8; e += THREADS) {
      const int f = e >> 9, l = (e >> 3) & 63, p = e & 7;
      reinterpret_cast<_Float16 *>(&s_frag[f][l])[p] = frag_value<L>(F, f, l & 31, l >> 5, p);
    }
  }
  __syncthreads();
  const int h = lane >> 5, j = lane & 31;
  for (; tile < n_tiles; tile += tile_stride) {
    const int i = tile * 64 + lane;
    uint32_t feat[L];
    if (PLANES) {  // features were produced by k_encode_xcd (level-major planes)
#pragma unroll
      for (int l = 0; l < L; l++) feat[l] = i < V ? planes[(size_t)l * plane_stride + i] : 0u;
    } else {
      float xn[3] = {0.f, 0.f, 0.f};
      if (i < V) normalise(F, x, (size_t)i, xn);
      encode_all<L, NLDS, NDENSE>(F, s_tab, xn, feat);
    }
    if (SAVE && i < V) {
      uint4 *o = reinterpret_cast<uint4 *>(acts + (size_t)i * ACT_STRIDE);
#pragma unroll
      for (int q = 0; q < L / 4; q++) o[q] = make_uint4(feat[4 * q], feat[4 * q + 1], feat[4 * q + 2], feat[4 * q + 3]);
    }
    // exchange: lane j gives its upper-half levels to lane j+32 and receives that
    // lane's lower-half levels (see header)
#pragma unroll
    for (int q = 0; q < L / 2; q++) {
      auto r = __builtin_amdgcn_permlane32_swap(feat[q], feat[q + L / 2], false, false);
      feat[q] = r[0];
      feat[q + L / 2] = r[1];
    }
#pragma unroll
    for (int cb = 0; cb < 2; cb++) {
      floatx16 a1[2], a3[2], a4[2], a2, a5;
      // ---- sigma net layer 1: [64 x 2L] ----
#pragma unroll
      for (int rb = 0; rb < 2; rb++) {
        a1[rb] = (floatx16){0.f};
#pragma unroll
        for (int s = 0; s < L / 8; s++) {
          union { uint32_t u[4]; half8 v; } b;
#pragma unroll
          for (int q = 0; q < 4; q++) b.u[q] = feat[cb * (L / 2) + 4 * s + q];
          a1[rb] = MFMA(s_frag[F_SIG1 + rb * 2 + s][lane], b.v, a1[rb]);
        }
      }
      const int o = tile * 64 + cb * 32 + j;
      uint16_t *arow = SAVE ? acts + (size_t)o * ACT_STRIDE + 2 * L : nullptr;
      if (SAVE && o < V) { save_rows<4>(arow, a1[0], h, true); save_rows<4>(arow + 32, a1[1], h, true); }
      // ---- sigma net layer 2: [16 x 64] ----
      a2 = (floatx16){0.f};
#pragma unroll
      for (int s = 0; s < 4; s++)
        a2 = MFMA(s_frag[F_SIG2 + s][lane], (s & 1) ? pack_slab<true>(a1[s >> 1], 1) : pack_slab<true>(a1[s >> 1], 0), a2);
      if (SAVE && o < V) save_rows<2>(arow + 64, a2, h, false);
      half8 cin = pack_slab<false>(a2, 0);  // out[kk], kk = C/D rows 0..15
      const float sig = (float)cin[0];      // row 0 lives in lanes h == 0
      if (h == 0) cin[0] = (_Float16)1.0f;  // identity-encoding padding constant
      // ---- colour net ----
#pragma unroll
      for (int rb = 0; rb < 2; rb++) a3[rb] = MFMA(s_frag[F_COL1 + rb][lane], cin, (floatx16){0.f});
      if (SAVE && o < V) { save_rows<4>(arow + 80, a3[0], h, true); save_rows<4>(arow + 112, a3[1], h, true); }
#pragma unroll
      for (int rb = 0; rb < 2; rb++) {
        a4[rb] = (floatx16){0.f};
#pragma unroll
        for (int s = 0; s < 4; s++)
          a4[rb] = MFMA(s_frag[F_COL2 + rb * 4 + s][lane],
                        (s & 1) ? pack_slab<true>(a3[s >> 1], 1) : pack_slab<true>(a3[s >> 1], 0), a4[rb]);
      }
      if (SAVE && o < V) { save_rows<4>(arow + 144, a4[0], h, true); save_rows<4>(arow + 176, a4[1], h, true); }
      a5 = (floatx16){0.f};
#pragma unroll
      for (int s = 0; s < 4; s++)
        a5 = MFMA(s_frag[F_COL3 + s][lane], (s & 1) ? pack_slab<true>(a4[s >> 1], 1) : pack_slab<true>(a4[s >> 1], 0), a5);
      if (h == 0 && o < V) {
        sigma[o] = sig;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const float sg = 1.0f / (1.0f + expf(-a5[c]));  // tcnn logistic
          rgb[(size_t)o * 3 + c] = (float)(_Float16)sg;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Backward A-fragments (transposed weights).  The backward data path mirrors the forward chain:
//   dY --Wc3^T--> dC2 --Wc2^T--> dC1 --Wc1^T--> d(colour input) -> dO --W2^T--> dH1 --W1^T--> dF
// and again the C/D registers of one product are the B operand of the next, so the same
// k-permutation kk = (p&3) + 8(p>>2) + 4h is folded into the (transposed) weight fragments.
// ---------------------------------------------------------------------------
#define N_FRAG_BWD 20
#define B_C3 0   // [rb(2)]       dC2 rows, k = dY row (natural order 8h+p)
#define B_C2 2   // [rb(2)][s(4)] dC1 rows, k = dC2 row
#define B_C1 10  // [s(4)]        colour-input slot rows (slot t>=1 <-> out[t] = column t-1 of Wc1), k = dC1 row
#define B_S2 14  // [rb(2)]       dH1 rows, k = dO row
#define B_S1 16  // [s(4)]        dF rows (features), k = dH1 row

template <int L>
__device__ _Float16 frag_value_bwd(const FieldDev &F, int f, int i, int h, int p) {
  constexpr int NF = 2 * L;
  const int kk = (p & 3) + 8 * (p >> 2) + 4 * h;
  if (f < B_C2) return ld_h(F.col_w3, (8 * h + p) * 64 + f * 32 + i);
  if (f < B_C1) {
    const int rb = (f - B_C2) >> 2, sl = (f - B_C2) & 3;
    return ld_h(F.col_w2, (16 * sl + kk) * 64 + rb * 32 + i);
  }
  if (f < B_S2) {
    const int sl = f - B_C1;
    return (i >= 1 && i < 16) ? ld_h(F.col_w1, (16 * sl + kk) * 16 + (i - 1)) : (_Float16)0.f;
  }
  if (f < B_S1) return ld_h(F.sig_w2, kk * 64 + (f - B_S2) * 32 + i);
  const int sl = f - B_S1;
  return i < NF ? ld_h(F.sig_w1, (16 * sl + kk) * NF + i) : (_Float16)0.f;
}

// Builds the MFMA A-fragment images [N_FRAG + N_FRAG_BWD][64 lanes][8 halves] once per weight update.
template <int L>
__global__ __launch_bounds__(256) void k_build_frags(FieldDev F, uint16_t *__restrict__ out) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < (N_FRAG + N_FRAG_BWD) * 64 * 8; e += gridDim.x * blockDim.x) {
    const int f = e >> 9, l = (e >> 3) & 63, p = e & 7;
    union { uint16_t u; _Float16 h; } c;
    c.h = f < N_FRAG ? frag_value<L>(F, f, l & 31, l >> 5, p) : frag_value_bwd<L>(F, f - N_FRAG, l & 31, l >> 5, p);
    out[e] = c.u;
  }
}

extern "C" size_t ia_field_frags_bytes(void) { return (size_t)(N_FRAG + N_FRAG_BWD) * 64 * 8 * 2; }

extern "C" int ia_field_prepare(const ia_field *field, uint16_t *frags_out, void *stream) {
  IA_CHECK_ARG(frags_out, "ia_field_prepare: null output");
  FieldDev F;
  int rc = ia_make_field_dev(field, &F);
  IA_CHECK_ARG(rc == 0, "ia_field_prepare: bad field descriptor (%d)", rc);
  F.frags = nullptr;
  if (F.lv.n_levels == 16)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_build_frags<16>), dim3(84), dim3(256), 0, (hipStream_t)stream, F, frags_out);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_build_frags<8>), dim3(84), dim3(256), 0, (hipStream_t)stream, F, frags_out);
  IA_LAUNCH_CHECK("k_build_frags");
  return IA_OK;
}

// Encoding only: feat fp16 [V,32] level-major (tcnn output order).
template <int L>
__global__ __launch_bounds__(256) void k_hashgrid(const float *__restrict__ x, int V, FieldDev F,
                                                  uint32_t *__restrict__ feat) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < V; i += gridDim.x * blockDim.x) {
    float xn[3];
    normalise(F, x, (size_t)i, xn);
    uint32_t f[L];
    encode_all<L, 0, -1>(F, nullptr, xn, f);
    uint4 *o = reinterpret_cast<uint4 *>(feat + (size_t)i * L);
#pragma unroll
    for (int q = 0; q < L / 4; q++) o[q] = make_uint4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
  }
}

#ifndef IA_SHARD_MIN
#define IA_SHARD_MIN 8192  // below this a call is launch-latency bound: one fused kernel
#endif

int ia_launch_field(const float *x, int V, const int32_t *n_dev, const FieldDev &F, float *rgb,
                    float *sigma, hipStream_t s, uint16_t *acts) {
  if (V <= 0) return IA_OK;
  const int tiles = (V + 63) / 64;
  int blocks = tiles < 256 ? tiles : 256;  // one workgroup per CU; waves loop over tiles
  // specialisation: leading dense levels (tcnn default: 4), the first two of them staged in LDS
  int n_dense = 0;
  while (n_dense < F.lv.n_levels && !F.lv.hashed[n_dense]) n_dense++;
  bool pattern = n_dense == 4 && F.hash_size != 0 && (int)F.n_dense == n_dense;
  const bool sharded = F.enc_ws && (size_t)V <= F.enc_ws_samples && V >= IA_SHARD_MIN && ia_field_shardable(F);
  const int lds_entries = (pattern && !sharded) ? (int)((F.lv.offset[2] + 3) / 4 * 4) : 0;
  pattern = pattern && (size_t)lds_entries * 4 <= 72 * 1024 && F.lv.offset[0] == 0;
  const size_t shmem = (size_t)N_FRAG * 64 * 16 + (pattern ? (size_t)lds_entries * 4 : 0);
  static bool attr_done = false;
  if (!attr_done) {  // > 64 KB of dynamic LDS must be opted into once per kernel
    const int lim = 160 * 1024;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_field<16, true, 2, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, lim);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_field<8, true, 2, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, lim);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_field<16, false, 2, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, lim);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_field<8, false, 2, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, lim);
    attr_done = true;
  }
  unsigned long long *prof = ia_prof_units(IA_PROF_FIELD);
  ia_prof_begin(IA_PROF_FIELD, s);
  dim3 g(blocks), b(IA_FIELD_THREADS);
  const int L16 = F.lv.n_levels == 16;
  const uint32_t *planes = nullptr;
  const size_t stride = F.enc_ws_samples;
#define IA_LF(LV, SV, NL, ND, PL) \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_field<LV, SV, NL, ND, PL>), g, b, shmem, s, x, V, n_dev, F, rgb, sigma, prof, acts, \
                     pattern ? lds_entries : 0, planes, stride)
  if (sharded) {
    int rc = ia_launch_encode_xcd(x, V, n_dev, F, F.enc_ws, stride, s, acts ? IA_ENC_S : IA_ENC_S_RENDER);
    if (rc != IA_OK) return rc;
    planes = F.enc_ws;
    if (!acts) {  // one-wave-per-SIMD workgroups, IA_FIELD_PLANES_WG_PER_CU per CU (a workgroup without a tile returns at once)
      const int cap = 256 * IA_FIELD_PLANES_WG_PER_CU;
      g = dim3(tiles < cap ? tiles : cap);
      b = dim3(field_threads(false, true));
    }
    if (acts) { if (L16) IA_LF(16, true, 0, 4, true); else IA_LF(8, true, 0, 4, true); }
    else { if (L16) IA_LF(16, false, 0, 4, true); else IA_LF(8, false, 0, 4, true); }
  } else if (pattern) {
    if (acts) { if (L16) IA_LF(16, true, 2, 4, false); else IA_LF(8, true, 2, 4, false); }
    else { if (L16) IA_LF(16, false, 2, 4, false); else IA_LF(8, false, 2, 4, false); }
  } else {
    if (acts) { if (L16) IA_LF(16, true, 0, -1, false); else IA_LF(8, true, 0, -1, false); }
    else { if (L16) IA_LF(16, false, 0, -1, false); else IA_LF(8, false, 0, -1, false); }
  }
#undef IA_LF
  ia_prof_end(IA_PROF_FIELD, s);
  IA_LAUNCH_CHECK("k_field");
  return IA_OK;
}

extern "C" int ia_field_fwd(const float *x, int V, const int32_t *n_dev, const ia_field *field, float *rgb,
                            float *sigma, void *stream) {
  IA_CHECK_ARG(V >= 0, "ia_field_fwd: V < 0");
  if (V == 0) return IA_OK;
  IA_CHECK_ARG(x && rgb && sigma, "ia_field_fwd: null pointer");
  FieldDev F;
  int rc = ia_make_field_dev(field, &F);
  IA_CHECK_ARG(rc == 0, "ia_field_fwd: bad field descriptor (%d)", rc);
  return ia_launch_field(x, V, n_dev, F, rgb, sigma, (hipStream_t)stream, nullptr);
}

// Training-mode forward: additionally writes the fp16 activation record per sample.
extern "C" int ia_field_act_stride(int n_levels) { return 2 * n_levels + 64 + 16 + 64 + 64; }

extern "C" int ia_field_fwd_train(const float *x, int V, const int32_t *n_dev, const ia_field *field, float *rgb,
                                  float *sigma, uint16_t *acts, void *stream) {
  IA_CHECK_ARG(V >= 0, "ia_field_fwd_train: V < 0");
  if (V == 0) return IA_OK;
  IA_CHECK_ARG(x && rgb && sigma && acts, "ia_field_fwd_train: null pointer");
  FieldDev F;
  int rc = ia_make_field_dev(field, &F);
  IA_CHECK_ARG(rc == 0, "ia_field_fwd_train: bad field descriptor (%d)", rc);
  return ia_launch_field(x, V, n_dev, F, rgb, sigma, (hipStream_t)stream, acts);
}


// ---------------------------------------------------------------------------
// Fused MLP backward (tcnn FullyFusedMLP backward for both networks): from the fp16 activation
// record of ia_field_fwd_train and dL/d(rgb, sigma) it produces dL/d(features) [V,2L] fp32 and
// accumulates the five weight gradients (fp32) -- one kernel instead of ten GEMM launches whose
// reduction dimension is the sample count (K = V, M,N <= 64: a shape GEMM libraries serve badly).
//
// One wave owns a tile of 32 samples per step.
//   * data path: MFMA 32x32x16 f16 chain as in the forward kernel, transposed weight fragments;
//     ReLU masks come from the saved activations, loaded in the C/D register layout;
//   * weight gradients dW = G A^T contract over SAMPLES, which sit across lanes in the C/D layout:
//     gradients G and activations A are staged once per tile in LDS as [row][sample] so that an
//     MFMA operand (row i, 8 consecutive samples) is one ds_read_b128; the 12 output tiles
//     (192 fp32 accumulators) stay in registers over all tiles of the wave and are reduced
//     through LDS and one round of global atomics at the end.
// Gradients are scaled by *scale (chosen by the caller so that the largest incoming gradient is
// 2^10) before they are rounded to half, and the scale is divided out of every fp32 result.
// ---------------------------------------------------------------------------
#define IA_BWD_THREADS 128
#define IA_BWD_RS 32  // halves per staged row = the 32 samples of a tile (59 KB of stage per workgroup: two per CU)
// staged rows
#define R_GY 0
#define R_GC2 16
#define R_GC1 80
#define R_GO 144
#define R_GH1 160
#define R_AC2 224
#define R_AC1 288
#define R_ACIN 352
#define R_AH1 368
#define R_AF 432
#define R_TOTAL 464

// 4 consecutive rows (8g + 4h + q) of a saved activation -> 4 halves
__device__ __forceinline__ void load4(const uint16_t *__restrict__ rec, int off, bool valid, _Float16 *o) {
  union { uint2 u; _Float16 h[4]; } c;
  c.u = valid ? *reinterpret_cast<const uint2 *>(rec + off) : make_uint2(0u, 0u);
#pragma unroll
  for (int q = 0; q < 4; q++) o[q] = c.h[q];
}

__device__ __forceinline__ half8 pack8(const _Float16 *g, int sub) {
  half8 o;
#pragma unroll
  for (int p = 0; p < 8; p++) o[p] = g[8 * sub + p];
  return o;
}

template <int L>
__global__ __launch_bounds__(IA_BWD_THREADS) void k_field_bwd(
    const uint16_t *__restrict__ acts, const float *__restrict__ rgb, const float *__restrict__ d_rgb,
    const float *__restrict__ d_sigma, int V, const int32_t *__restrict__ n_dev, const float *__restrict__ scale,
    const uint16_t *__restrict__ frags, float *__restrict__ dfeat, float *__restrict__ partial) {
  constexpr int NF = 2 * L, STRIDE = NF + 208, RS = IA_BWD_RS, NW = IA_BWD_THREADS / 64;
  constexpr int O_H1 = NF, O_O = NF + 64, O_C1 = NF + 80, O_C2 = NF + 144;
  extern __shared__ __attribute__((aligned(16))) char s_dyn[];
  half8 (*s_frag)[64] = reinterpret_cast<half8 (*)[64]>(s_dyn);
  if (n_dev) V = min(V, *n_dev);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  _Float16 *st = reinterpret_cast<_Float16 *>(s_dyn + N_FRAG_BWD * 64 * 16) + (size_t)wave * R_TOTAL * RS;
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(frags + (size_t)N_FRAG * 64 * 8);
    uint4 *dst = reinterpret_cast<uint4 *>(&s_frag[0][0]);
    for (int e = threadIdx.x; e < N_FRAG_BWD * 64; e += IA_BWD_THREADS) dst[e] = src[e];
  }
  // constant row of the colour input (identity-encoding padding, slot 15 of the 16 inputs)
  if (h == 0) st[(R_ACIN + 15) * RS + j] = (_Float16)1.0f;
  __syncthreads();
  const float S = *scale, invS = 1.0f / S;
  floatx16 aC3[2], aC2[4], aC1[2], aW2[2], aW1[2];
#pragma unroll
  for (int q = 0; q < 2; q++) { aC3[q] = (floatx16){0.f}; aC1[q] = (floatx16){0.f}; aW2[q] = (floatx16){0.f}; aW1[q] = (floatx16){0.f}; }
#pragma unroll
  for (int q = 0; q < 4; q++) aC2[q] = (floatx16){0.f};
  const int n_tiles = (V + 31) >> 5;
  const half8 zero8 = (half8){(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f,
                              (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
  for (int t0 = blockIdx.x * NW; t0 < n_tiles; t0 += gridDim.x * NW) {  // uniform trip count per workgroup
    const int tile = t0 + wave;
    const int n = tile * 32 + j;
    const bool valid = tile < n_tiles && n < V;
    const uint16_t *rec = acts + (size_t)(valid ? n : 0) * STRIDE;
    // ---- saved activations in the C/D layout (rows 8g + 4h + q <-> register 4g + q) ----
    _Float16 c2v[2][16], c1v[2][16], h1v[2][16], ov[8], fv[16];
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        load4(rec, O_C2 + b * 32 + 8 * g + 4 * h, valid, &c2v[b][4 * g]);
        load4(rec, O_C1 + b * 32 + 8 * g + 4 * h, valid, &c1v[b][4 * g]);
        load4(rec, O_H1 + b * 32 + 8 * g + 4 * h, valid, &h1v[b][4 * g]);
      }
#pragma unroll
    for (int g = 0; g < 2; g++) load4(rec, O_O + 8 * g + 4 * h, valid, &ov[4 * g]);
#pragma unroll
    for (int g = 0; g < NF / 8; g++) load4(rec, 8 * g + 4 * h, valid, &fv[4 * g]);
    // stage the activations as [row][sample]
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = b * 32 + cd_row(r, h);
        st[(R_AC2 + row) * RS + j] = c2v[b][r];
        st[(R_AC1 + row) * RS + j] = c1v[b][r];
        st[(R_AH1 + row) * RS + j] = h1v[b][r];
      }
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const int row = cd_row(r, h);              // sigma-net output row; colour input m = row - 1
      if (row >= 1) st[(R_ACIN + row - 1) * RS + j] = ov[r];
    }
#pragma unroll
    for (int r = 0; r < NF / 2; r++) st[(R_AF + cd_row(r, h)) * RS + j] = fv[r];
    // ---- dY = dL/drgb * sigmoid' (rows 0..2), natural k order: lanes h == 0 hold k = 0..7 ----
    half8 by = zero8;
    if (h == 0 && valid) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float y = rgb[(size_t)n * 3 + c];
        by[c] = (_Float16)(d_rgb[(size_t)n * 3 + c] * y * (1.0f - y) * S);
      }
    }
#pragma unroll
    for (int p = 0; p < 8; p++) st[(R_GY + 8 * h + p) * RS + j] = by[p];
    // ---- dC2 = Wc3^T dY, masked by C2 > 0 ----
    _Float16 g2[2][16], g1[2][16], gh[2][16], go[8];
#pragma unroll
    for (int rb = 0; rb < 2; rb++) {
      const floatx16 a = MFMA(s_frag[B_C3 + rb][lane], by, (floatx16){0.f});
#pragma unroll
      for (int r = 0; r < 16; r++) {
        g2[rb][r] = c2v[rb][r] > (_Float16)0.f ? (_Float16)a[r] : (_Float16)0.f;
        st[(R_GC2 + rb * 32 + cd_row(r, h)) * RS + j] = g2[rb][r];
      }
    }
    // ---- dC1 = Wc2^T dC2, masked by C1 > 0 ----
#pragma unroll
    for (int rb = 0; rb < 2; rb++) {
      floatx16 a = (floatx16){0.f};
#pragma unroll
      for (int sl = 0; sl < 4; sl++) a = MFMA(s_frag[B_C2 + rb * 4 + sl][lane], pack8(g2[sl >> 1], sl & 1), a);
#pragma unroll
      for (int r = 0; r < 16; r++) {
        g1[rb][r] = c1v[rb][r] > (_Float16)0.f ? (_Float16)a[r] : (_Float16)0.f;
        st[(R_GC1 + rb * 32 + cd_row(r, h)) * RS + j] = g1[rb][r];
      }
    }
    // ---- d(colour input slots) = Wc1^T dC1; dO = [d sigma, d out[1..15]] ----
    {
      floatx16 a = (floatx16){0.f};
#pragma unroll
      for (int sl = 0; sl < 4; sl++) a = MFMA(s_frag[B_C1 + sl][lane], pack8(g1[sl >> 1], sl & 1), a);
#pragma unroll
      for (int r = 0; r < 8; r++) go[r] = (_Float16)a[r];
      if (h == 0) go[0] = valid ? (_Float16)(d_sigma[n] * S) : (_Float16)0.f;  // row 0 = sigma
#pragma unroll
      for (int r = 0; r < 8; r++) st[(R_GO + cd_row(r, h)) * RS + j] = go[r];
    }
    // ---- dH1 = W2^T dO, masked by H1 > 0 ----
#pragma unroll
    for (int rb = 0; rb < 2; rb++) {
      const floatx16 a = MFMA(s_frag[B_S2 + rb][lane], pack8(go, 0), (floatx16){0.f});
#pragma unroll
      for (int r = 0; r < 16; r++) {
        gh[rb][r] = h1v[rb][r] > (_Float16)0.f ? (_Float16)a[r] : (_Float16)0.f;
        st[(R_GH1 + rb * 32 + cd_row(r, h)) * RS + j] = gh[rb][r];
      }
    }
    // ---- dF = W1^T dH1 -> global fp32 [V][NF] ----
    {
      floatx16 a = (floatx16){0.f};
#pragma unroll
      for (int sl = 0; sl < 4; sl++) a = MFMA(s_frag[B_S1 + sl][lane], pack8(gh[sl >> 1], sl & 1), a);
      if (valid) {
#pragma unroll
        for (int g = 0; g < NF / 8; g++)
          *reinterpret_cast<float4 *>(dfeat + (size_t)n * NF + 8 * g + 4 * h) =
              make_float4(a[4 * g] * invS, a[4 * g + 1] * invS, a[4 * g + 2] * invS, a[4 * g + 3] * invS);
      }
    }
    __syncthreads();  // staged rows visible to the whole wave (lanes read other lanes' rows)
    // ---- weight gradients: dW[m][p] += sum_samples G[m][n] A[p][n] ----
    const int i = j;
#pragma unroll
    for (int sl = 0; sl < 2; sl++) {
      const int ko = 16 * sl + 8 * h;
      auto row8 = [&](int row) { return *reinterpret_cast<const half8 *>(st + (size_t)row * RS + ko); };
      const half8 gY = i < 16 ? row8(R_GY + i) : zero8, gO = i < 16 ? row8(R_GO + i) : zero8;
      const half8 aCin = i < 16 ? row8(R_ACIN + i) : zero8, aF = i < NF ? row8(R_AF + i) : zero8;
      half8 gC2[2], gC1[2], gH1[2], aC2r[2], aC1r[2], aH1r[2];
#pragma unroll
      for (int b = 0; b < 2; b++) {
        gC2[b] = row8(R_GC2 + b * 32 + i); gC1[b] = row8(R_GC1 + b * 32 + i); gH1[b] = row8(R_GH1 + b * 32 + i);
        aC2r[b] = row8(R_AC2 + b * 32 + i); aC1r[b] = row8(R_AC1 + b * 32 + i); aH1r[b] = row8(R_AH1 + b * 32 + i);
      }
#pragma unroll
      for (int b = 0; b < 2; b++) {
        aC3[b] = MFMA(gY, aC2r[b], aC3[b]);       // dWc3 [16][64]
        aW2[b] = MFMA(gO, aH1r[b], aW2[b]);       // dW2  [16][64]
        aC1[b] = MFMA(gC1[b], aCin, aC1[b]);      // dWc1 [64][16]
        aW1[b] = MFMA(gH1[b], aF, aW1[b]);        // dW1  [64][NF]
#pragma unroll
        for (int pb = 0; pb < 2; pb++) aC2[b * 2 + pb] = MFMA(gC2[b], aC1r[pb], aC2[b * 2 + pb]);  // dWc2 [64][64]
      }
    }
    __syncthreads();  // operands consumed before the next tile overwrites the stage
  }
  // ---- reduce the waves of the workgroup in LDS, then one round of global atomics ----
  float *red = reinterpret_cast<float *>(s_dyn + N_FRAG_BWD * 64 * 16);  // stage area reused
  constexpr int N_W1 = 64 * NF, N_W2 = 1024, N_C1 = 1024, N_C2 = 4096, N_C3 = 1024;
  constexpr int O_W1 = 0, O_W2 = O_W1 + N_W1, O_C1g = O_W2 + N_W2, O_C2g = O_C1g + N_C1, O_C3g = O_C2g + N_C2,
                N_ALL = O_C3g + N_C3;
  for (int e = threadIdx.x; e < N_ALL; e += IA_BWD_THREADS) red[e] = 0.f;
  __syncthreads();
  const int col = j;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int row = cd_row(r, h);
#pragma unroll
    for (int b = 0; b < 2; b++) {
      if (row < 16) {
        atomicAdd(&red[O_C3g + row * 64 + b * 32 + col], aC3[b][r]);
        atomicAdd(&red[O_W2 + row * 64 + b * 32 + col], aW2[b][r]);
      }
      if (col < 16) atomicAdd(&red[O_C1g + (b * 32 + row) * 16 + col], aC1[b][r]);
      if (col < NF) atomicAdd(&red[O_W1 + (b * 32 + row) * NF + col], aW1[b][r]);
#pragma unroll
      for (int pb = 0; pb < 2; pb++) atomicAdd(&red[O_C2g + (b * 32 + row) * 64 + pb * 32 + col], aC2[b * 2 + pb][r]);
    }
  }
  __syncthreads();
  // per-workgroup partial sums (scaled gradients); k_field_bwd_reduce adds them up in workgroup order:
  // no global atomics, bitwise reproducible weight gradients
  for (int e = threadIdx.x; e < N_ALL; e += IA_BWD_THREADS) partial[(size_t)blockIdx.x * N_ALL + e] = red[e];
}

// 256 threads = 32 gradient elements x 8 slices of the workgroup range: every thread adds up its slice
// (independent loads, 8 in flight), the slices are combined through LDS in slice order -> the sum
// order is fixed, the result bitwise reproducible.
template <int L>
__global__ __launch_bounds__(256) void k_field_bwd_reduce(const float *__restrict__ partial, int n_blocks,
                                                          const float *__restrict__ scale, float *__restrict__ g_w1,
                                                          float *__restrict__ g_w2, float *__restrict__ g_c1,
                                                          float *__restrict__ g_c2, float *__restrict__ g_c3) {
  constexpr int NF = 2 * L;
  constexpr int N_W1 = 64 * NF, N_W2 = 1024, N_C1 = 1024, N_C2 = 4096, N_C3 = 1024;
  constexpr int O_W2 = N_W1, O_C1g = O_W2 + N_W2, O_C2g = O_C1g + N_C1, O_C3g = O_C2g + N_C2, N_ALL = O_C3g + N_C3;
  __shared__ float s_part[8][32];
  const int el = threadIdx.x & 31, slice = threadIdx.x >> 5;
  const int e = blockIdx.x * 32 + el;  // N_ALL is a multiple of 32
  const int per = (n_blocks + 7) / 8, b0 = slice * per, b1 = min(b0 + per, n_blocks);
  float acc = 0.f;
#pragma unroll 8
  for (int b = b0; b < b1; b++) acc += partial[(size_t)b * N_ALL + e];
  s_part[slice][el] = acc;
  __syncthreads();
  if (slice != 0) return;
  float tot = 0.f;
#pragma unroll
  for (int k = 0; k < 8; k++) tot += s_part[k][el];
  float *dst = e < O_W2 ? g_w1 + e : e < O_C1g ? g_w2 + (e - O_W2) : e < O_C2g ? g_c1 + (e - O_C1g)
               : e < O_C3g ? g_c2 + (e - O_C2g) : g_c3 + (e - O_C3g);
  *dst += tot * (1.0f / *scale);
}

// Per-call gradient scale of the fused MLP backward: S = 1024 / max(|dL/drgb * rgb (1 - rgb)|, |dL/dsigma|) over the
// LIVE samples (tcnn relies on a fixed 1024x loss scale, DNeRF.py:58; here the largest incoming gradient is placed at
// 2^10 before the cast to half).  One launch, no host read: block maxima meet in an atomicMax on the float's bit
// pattern (non-negative floats order like integers), the last block to arrive (ticket) writes S and leaves the two
// state words zero for the next call.  Replaces five elementwise / reduction launches over the capacity-sized buffers.
__global__ __launch_bounds__(256) void k_grad_scale(const float *__restrict__ rgb, const float *__restrict__ d_rgb,
                                                    const float *__restrict__ d_sigma, int V, const int32_t *__restrict__ n_dev,
                                                    uint32_t *__restrict__ state /*[2]: max bits, tickets*/, float *__restrict__ scale) {
  if (n_dev) V = min(V, *n_dev);
  float m = 0.f;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < V; i += gridDim.x * blockDim.x) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float y = rgb[(size_t)i * 3 + c];
      const float g = fabsf(d_rgb[(size_t)i * 3 + c] * y * (1.0f - y));
      m = (g > m || isnan(g)) ? g : m;   // NaN propagates: the step is skipped by the non-finite check downstream
    }
    const float gs = fabsf(d_sigma[i]);
    m = (gs > m || isnan(gs)) ? gs : m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const float t = __shfl_xor(m, o, 64); m = (t > m || isnan(t)) ? t : m; }
  __shared__ float s_m[4];
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) m = (s_m[w] > m || isnan(s_m[w])) ? s_m[w] : m;
    atomicMax(&state[0], isnan(m) ? 0x7fc00000u : __float_as_uint(m));   // NaN's bit pattern is above every finite value's
    __threadfence();
    const uint32_t t = atomicAdd(&state[1], 1u);
    if (t == gridDim.x - 1) {
      const float amax = __uint_as_float(atomicExch(&state[0], 0u));
      atomicExch(&state[1], 0u);
      // a non-finite gradient makes the scale NaN: every half gradient, every weight-gradient sum and every table
      // contribution of this call become NaN and the step is skipped by the non-finite check downstream
      // (fmaxf(NaN, 1e-30f) would return 1e-30 -- S = 1e33, finite -- and an infinite amax would give S = 0)
      *scale = (isnan(amax) || isinf(amax)) ? __uint_as_float(0x7fc00000u) : 1024.0f / fmaxf(amax, 1e-30f);
    }
  }
}

extern "C" int ia_field_grad_scale(const float *rgb, const float *d_rgb, const float *d_sigma, int V, const int32_t *n_dev,
                                   uint32_t *state2, float *scale, void *stream) {
  IA_CHECK_ARG(V >= 0 && state2 && scale, "ia_field_grad_scale: bad arguments");
  IA_CHECK_ARG(V == 0 || (rgb && d_rgb && d_sigma), "ia_field_grad_scale: null pointer");
  int blocks = (V + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 256 ? 256 : blocks);
  hipLaunchKernelGGL(k_grad_scale, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rgb, d_rgb, d_sigma, V, n_dev, state2, scale);
  IA_LAUNCH_CHECK("k_grad_scale");
  return IA_OK;
}

static int ia_field_bwd_nblocks(int V) {
  const int n_tiles = (V + 31) / 32, per = IA_BWD_THREADS / 64;
  int nb = (n_tiles + per - 1) / per;
  if (nb > 512) nb = 512;  // two workgroups per CU; waves keep their 192 accumulators over all their tiles
  return nb < 1 ? 1 : nb;
}

extern "C" size_t ia_field_bwd_workspace_bytes(int V, int n_levels) {
  return (size_t)ia_field_bwd_nblocks(V) * (size_t)(64 * 2 * n_levels + 1024 + 1024 + 4096 + 1024) * sizeof(float);
}

extern "C" int ia_field_bwd(const uint16_t *acts, const float *rgb, const float *d_rgb, const float *d_sigma, int V,
                            const int32_t *n_dev, const float *scale, const ia_field *field, float *dfeat, float *g_sig_w1,
                            float *g_sig_w2, float *g_col_w1, float *g_col_w2, float *g_col_w3, void *ws, size_t ws_bytes,
                            void *stream) {
  IA_CHECK_ARG(V >= 0, "ia_field_bwd: V < 0");
  if (V == 0) return IA_OK;
  IA_CHECK_ARG(acts && rgb && d_rgb && d_sigma && scale && dfeat && g_sig_w1 && g_sig_w2 && g_col_w1 && g_col_w2 && g_col_w3,
               "ia_field_bwd: null pointer");
  FieldDev F;
  int rc = ia_make_field_dev(field, &F);
  IA_CHECK_ARG(rc == 0, "ia_field_bwd: bad field descriptor (%d)", rc);
  IA_CHECK_ARG(F.frags, "ia_field_bwd: field.mlp_frags is required (ia_field_prepare)");
  const size_t shmem = (size_t)N_FRAG_BWD * 64 * 16 + (size_t)(IA_BWD_THREADS / 64) * R_TOTAL * IA_BWD_RS * 2;
  static bool attr_done = false;
  if (!attr_done) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_field_bwd<16>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_field_bwd<8>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_done = true;
  }
  const int blocks = ia_field_bwd_nblocks(V);
  IA_CHECK_ARG(ws != nullptr, "ia_field_bwd: null workspace");
  if (ws_bytes < ia_field_bwd_workspace_bytes(V, F.lv.n_levels)) return ia_set_error(IA_ERR_WORKSPACE, "ia_field_bwd: workspace too small");
  float *partial = static_cast<float *>(ws);
  const int n_all = 64 * 2 * F.lv.n_levels + 1024 + 1024 + 4096 + 1024;
  if (F.lv.n_levels == 16) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_field_bwd<16>), dim3(blocks), dim3(IA_BWD_THREADS), shmem, (hipStream_t)stream, acts, rgb,
                       d_rgb, d_sigma, V, n_dev, scale, F.frags, dfeat, partial);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_field_bwd_reduce<16>), dim3(n_all / 32), dim3(256), 0, (hipStream_t)stream,
                       partial, blocks, scale, g_sig_w1, g_sig_w2, g_col_w1, g_col_w2, g_col_w3);
  } else {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_field_bwd<8>), dim3(blocks), dim3(IA_BWD_THREADS), shmem, (hipStream_t)stream, acts, rgb,
                       d_rgb, d_sigma, V, n_dev, scale, F.frags, dfeat, partial);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_field_bwd_reduce<8>), dim3(n_all / 32), dim3(256), 0, (hipStream_t)stream,
                       partial, blocks, scale, g_sig_w1, g_sig_w2, g_col_w1, g_col_w2, g_col_w3);
  }
  IA_LAUNCH_CHECK("k_field_bwd");
  return IA_OK;
}

// ---------------------------------------------------------------------------
// Hash-grid backward (tcnn kernel_grid_backward / kernel_grid_backward_input):
// dL/dtable[entry][f] += w_corner * dL/dfeat[level][f]   (fp32 atomics)
// dL/dx (optional)     = sum_levels scale_l * sum_corners dw/dpos * <val, dfeat>
// One lane = one sample; the level loop is wave-uniform.
// ---------------------------------------------------------------------------
// Samples arrive ray-major: consecutive lanes are consecutive samples of one ray, and on the coarse levels a run of
// lanes falls into the SAME cell (level 0: ~20 samples per cell).  Left alone, the wave then fires up to 64 atomics
// at each of the cell's 16 words and the L2 serialises them: level 0 alone cost 20x a fine level (2.9 ms against
// 0.14 ms for 180 k samples with dense gradients).  On levels < IA_HGB_REDUCE_LEVELS every run of consecutive lanes
// with the same cell is summed inside the wave first (segmented suffix sum by doubling: 6 shuffle steps per value,
// run structure computed once per level) and only the head lane of a run issues the atomics.
#ifndef IA_HGB_REDUCE_LEVELS
#define IA_HGB_REDUCE_LEVELS 8
#endif

// one round of the quad-cooperative scatter: every lane of a quad reads the operands of quad lane R (DPP quad_perm) and
// adds its own word of that sample's (x0, x1) entry pair
template <int R>
__device__ __forceinline__ void ia_hgb_quad_round(float *__restrict__ dtab, int qj, uint32_t i0, uint32_t i1, float q0, float q1,
                                                  float q2, float q3) {
  constexpr int CTRL = R * 0x55;   // quad_perm [R, R, R, R]
#define IA_QB_I(v) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), CTRL, 0xF, 0xF, false))
#define IA_QB_F(v) (__int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false)))
  const uint32_t b0 = IA_QB_I(i0), b1 = IA_QB_I(i1);
  const float t0 = IA_QB_F(q0), t1 = IA_QB_F(q1), t2 = IA_QB_F(q2), t3 = IA_QB_F(q3);
#undef IA_QB_I
#undef IA_QB_F
  const uint32_t bi = (qj & 2) ? b1 : b0;
  const float val = (qj & 2) ? ((qj & 1) ? t3 : t2) : ((qj & 1) ? t1 : t0);
  if (val != 0.f) unsafeAtomicAdd(dtab + (size_t)bi * 2 + (qj & 1), val);
}

template <int L>
__global__ __launch_bounds__(256) void k_hashgrid_bwd(const float *__restrict__ x, int V,
                                                      const int32_t *__restrict__ n_dev, FieldDev F,
                                                      const float *__restrict__ dfeat,
                                                      float *__restrict__ dtable, float *__restrict__ dx,
                                                      int l_begin, int l_end) {
  if (n_dev) V = min(V, *n_dev);
  const int lane = threadIdx.x & 63;
  if (gridDim.y > 1) {  // level groups side by side (blockIdx.y): more waves per CU for the 10^5-sample calls of a training step
    const int nl = l_end - l_begin, lb = l_begin + nl * (int)blockIdx.y / (int)gridDim.y;
    l_end = l_begin + nl * ((int)blockIdx.y + 1) / (int)gridDim.y;
    l_begin = lb;
  }
  const int n_round = (V + (int)(gridDim.x * blockDim.x) - 1) / (int)(gridDim.x * blockDim.x);  // uniform trip count: shuffles below
  for (int rd = 0; rd < n_round; rd++) {
    const int i = rd * gridDim.x * blockDim.x + blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < V;
    float xn[3] = {0.f, 0.f, 0.f};
    if (live) normalise(F, x, (size_t)i, xn);
    float gx[3] = {0.f, 0.f, 0.f};
#ifndef IA_HGB_LEVEL_UNROLL
#define IA_HGB_LEVEL_UNROLL 1
#endif
#pragma unroll IA_HGB_LEVEL_UNROLL
    for (int l = l_begin; l < l_end; l++) {
      const float scale = F.lv.scale[l];
      const uint32_t res = F.lv.res[l], size = F.lv.size[l];
      const bool hashed = F.lv.hashed[l] != 0;
      const uint32_t *tab = F.table + F.lv.offset[l];
      float *dtab = dtable + (size_t)F.lv.offset[l] * 2;
      float d0 = 0.f, d1 = 0.f;
      if (live) { d0 = dfeat[(size_t)i * (2 * L) + 2 * l]; d1 = dfeat[(size_t)i * (2 * L) + 2 * l + 1]; }
      float w[3];
      uint32_t g[3];
#pragma unroll
      for (int d = 0; d < 3; d++) {   // pos_fract (ia_field_dev.h), spelled out: the call changes this unit's device code
        const float pos = __builtin_fmaf(xn[d], scale, 0.5f);
        const float fl = floorf(pos);
        g[d] = (uint32_t)(int)fl;
        w[d] = pos - fl;
      }
      // ---- run structure of this level (wave-uniform decision) ----
      const bool reduce = l < IA_HGB_REDUCE_LEVELS;
      uint32_t cont = 0u;   // bit k: the run of this lane's cell continues for at least 2^k more lanes
      bool head = true;
      if (reduce) {
        // cells are < 2^10 per axis on the reduced levels (level 7: 274); dead lanes get a key no live lane has
        const uint32_t key = live ? ((g[0] << 20) | (g[1] << 10) | g[2]) : (0xC0000000u | (uint32_t)lane);
        const uint32_t up = __shfl_up(key, 1, 64);
        head = lane == 0 || up != key;
        const uint32_t dn = __shfl_down(key, 1, 64);  // (every shuffle is executed by ALL lanes: no short-circuit in front of one)
        bool c = (lane + 1 < 64) && dn == key;
        cont = c ? 1u : 0u;
#pragma unroll
        for (int k = 1; k < 6; k++) {
          const int o = 1 << (k - 1);
          const int cn = __shfl_down((int)c, o, 64);
          c = c && (lane + o < 64) && (cn != 0);  // cont(2o) = cont(o) at i AND at i + o
          cont |= c ? (1u << k) : 0u;
        }
      }
      uint32_t c_index[8];
      float c_v0[8], c_v1[8];
#pragma unroll
      for (int idx = 0; idx < 8; idx++) {
        const uint32_t cx = g[0] + (idx & 1), cy = g[1] + ((idx >> 1) & 1), cz = g[2] + ((idx >> 2) & 1);
        uint32_t index;   // corner_index (ia_field_dev.h), spelled out for the same reason
        if (hashed) {
          index = (cx ^ (cy * 2654435761u) ^ (cz * 805459861u)) & (size - 1);
        } else {
          index = cx + cy * res + cz * res * res;
          if (index >= size) index -= size;
          index = min(index, size - 1);
        }
        const float wx = (idx & 1) ? w[0] : 1.f - w[0], wy = (idx & 2) ? w[1] : 1.f - w[1], wz = (idx & 4) ? w[2] : 1.f - w[2];
        const float wt = wx * wy * wz;
        float v0 = wt * d0, v1 = wt * d1;
        if (reduce) {
          // segmented suffix sum: after step k a lane holds the sum over min(2^(k+1), rest of its run) lanes
#pragma unroll
          for (int k = 0; k < 6; k++) {
            const float a0 = __shfl_down(v0, 1 << k, 64), a1 = __shfl_down(v1, 1 << k, 64);
            if ((cont >> k) & 1u) { v0 += a0; v1 += a1; }
          }
        }
        c_index[idx] = index;
        c_v0[idx] = (live && head) ? v0 : 0.f;   // zero = nothing to add (skipped below)
        c_v1[idx] = (live && head) ? v1 : 0.f;
        if (dx && live) {
          union { uint32_t u; half2v h; } c;
          c.u = tab[index];
          const float dot = (float)c.h.x * d0 + (float)c.h.y * d1;
          const float sx = (idx & 1) ? 1.f : -1.f, sy = (idx & 2) ? 1.f : -1.f, sz = (idx & 4) ? 1.f : -1.f;
          gx[0] += scale * sx * wy * wz * dot;
          gx[1] += scale * wx * sy * wz * dot;
          gx[2] += scale * wx * wy * sz * dot;
        }
      }
      // ---- quad-cooperative scatter -----------------------------------------------------------------------------------
      // The atomic units take ~21 G REQUESTS/s whatever they carry, and the lanes of one instruction that hit adjacent
      // words are one request (tools/ubench/atomics.hip: 21 / 42 / 84 G atomics/s for single words / pairs / 16-byte
      // quads).  So the four lanes of a quad serve ONE sample per round: lane j adds feature (j & 1) of the x-neighbour
      // (j >> 1) -- the two features of an entry are 8 contiguous bytes, and the x-neighbour's entry follows directly on
      // dense levels and on hashed levels when cx is even (the hash differs in bit 0 only): one or two requests per
      // (sample, y, z) instead of four.  Same additions, same operands; only which lane issues them changes.
      // (Measured on top of this and dropped: the coarse dense levels 0-2 accumulated per workgroup in LDS slabs by a
      // second kernel -- level 0 alone 222 -> 40 us, but the whole scatter 984 -> 966 us and the training step unchanged:
      // the same-address traffic of the coarse levels drains under the fine levels' requests, it is not on the critical path.)
      {
        const int qj = lane & 3;
#pragma unroll
        for (int yz = 0; yz < 4; yz++) {
          const uint32_t i0 = c_index[2 * yz], i1 = c_index[2 * yz + 1];
          const float q0 = c_v0[2 * yz], q1 = c_v1[2 * yz], q2 = c_v0[2 * yz + 1], q3 = c_v1[2 * yz + 1];
          ia_hgb_quad_round<0>(dtab, qj, i0, i1, q0, q1, q2, q3);
          ia_hgb_quad_round<1>(dtab, qj, i0, i1, q0, q1, q2, q3);
          ia_hgb_quad_round<2>(dtab, qj, i0, i1, q0, q1, q2, q3);
          ia_hgb_quad_round<3>(dtab, qj, i0, i1, q0, q1, q2, q3);
        }
      }
    }
    if (dx && live) {
#pragma unroll
      for (int d = 0; d < 3; d++) {
        // d xn / d x = 1/scale inside the unit cube, 0 where the clamp is active (ngp.py:75-77)
        const float raw = (x[(size_t)i * 3 + d] - F.center[d]) / F.scale[d] + 0.5f;
        dx[(size_t)i * 3 + d] = (raw > 0.f && raw < 1.f) ? gx[d] / F.scale[d] : 0.f;
      }
    }
  }
}

static int hashgrid_bwd_impl(const float *x, int V, const int32_t *n_dev, const ia_field *field, const float *dfeat,
                             float *dtable, float *dx, int l_begin, int l_end, void *stream, const char *who) {
  IA_CHECK_ARG(V >= 0, "%s: V < 0", who);
  if (V == 0) return IA_OK;
  IA_CHECK_ARG(x && dfeat && dtable, "%s: null pointer", who);
  FieldDev F;
  int rc = ia_make_field_dev(field, &F);
  IA_CHECK_ARG(rc == 0, "%s: bad field descriptor (%d)", who, rc);
  IA_CHECK_ARG(0 <= l_begin && l_begin < l_end && l_end <= F.lv.n_levels, "%s: bad level range [%d, %d)", who, l_begin, l_end);
  IA_CHECK_ARG(!dx || (l_begin == 0 && l_end == F.lv.n_levels), "%s: dx needs the full level range", who);
  int blocks = (V + 255) / 256;
  if (blocks > 4096) blocks = 4096;
#ifndef IA_HGB_LEVEL_GROUPS
#define IA_HGB_LEVEL_GROUPS 1  // level groups side by side in one launch; training it/s (r02, graph replay): 1 / 2 / 4 / 8 / 16 groups =
#endif                         // 1210 / 1175 / 1148 / 1146 / 1141 -- the scatter is bound by the atomics, not by occupancy
  // the input gradient sums over levels inside a thread: one group then
  int groups = dx ? 1 : IA_HGB_LEVEL_GROUPS;
  if (groups > l_end - l_begin) groups = l_end - l_begin;
  if (F.lv.n_levels == 16)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_hashgrid_bwd<16>), dim3(blocks, groups), dim3(256), 0, (hipStream_t)stream, x, V, n_dev, F, dfeat, dtable, dx, l_begin, l_end);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_hashgrid_bwd<8>), dim3(blocks, groups), dim3(256), 0, (hipStream_t)stream, x, V, n_dev, F, dfeat, dtable, dx, l_begin, l_end);
  IA_LAUNCH_CHECK("k_hashgrid_bwd");
  return IA_OK;
}

extern "C" int ia_hashgrid_bwd(const float *x, int V, const int32_t *n_dev, const ia_field *field, const float *dfeat,
                               float *dtable, float *dx, void *stream) {
  return hashgrid_bwd_impl(x, V, n_dev, field, dfeat, dtable, dx, 0, field ? field->hash.n_levels : 0, stream, "ia_hashgrid_bwd");
}

// The same scatter restricted to levels [l_begin, l_end): lets the caller hand a finished slice of the table
// gradient to the gradient all-reduce while the remaining levels are still being scattered.
extern "C" int ia_hashgrid_bwd_levels(const float *x, int V, const int32_t *n_dev, const ia_field *field, const float *dfeat,
                                      float *dtable, int l_begin, int l_end, void *stream) {
  return hashgrid_bwd_impl(x, V, n_dev, field, dfeat, dtable, nullptr, l_begin, l_end, stream, "ia_hashgrid_bwd_levels");
}

extern "C" int ia_hashgrid_fwd(const float *x, int V, const ia_field *field, uint16_t *feat, void *stream) {
  IA_CHECK_ARG(V >= 0, "ia_hashgrid_fwd: V < 0");
  if (V == 0) return IA_OK;
  IA_CHECK_ARG(x && feat, "ia_hashgrid_fwd: null pointer");
  FieldDev F;
  int rc = ia_make_field_dev(field, &F);
  IA_CHECK_ARG(rc == 0, "ia_hashgrid_fwd: bad field descriptor (%d)", rc);
  int blocks = (V + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (F.lv.n_levels == 16)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_hashgrid<16>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, V, F,
                       reinterpret_cast<uint32_t *>(feat));
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_hashgrid<8>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, V, F,
                       reinterpret_cast<uint32_t *>(feat));
  IA_LAUNCH_CHECK("k_hashgrid");
  return IA_OK;
}

// Encoding only, XCD-sharded: planes [n_levels][stride] of packed half2 (level-major).
extern "C" int ia_hashgrid_fwd_planes(const float *x, int V, const ia_field *field, uint32_t *planes, size_t stride,
                                      void *stream) {
  IA_CHECK_ARG(V >= 0, "ia_hashgrid_fwd_planes: V < 0");
  if (V == 0) return IA_OK;
  IA_CHECK_ARG(x && planes && stride >= (size_t)V, "ia_hashgrid_fwd_planes: null pointer or stride < V");
  FieldDev F;
  int rc = ia_make_field_dev(field, &F);
  IA_CHECK_ARG(rc == 0, "ia_hashgrid_fwd_planes: bad field descriptor (%d)", rc);
  IA_CHECK_ARG(ia_field_shardable(F), "ia_hashgrid_fwd_planes: level table is not 4 dense + 4/12 uniform hashed levels");
  return ia_launch_encode_xcd(x, V, nullptr, F, planes, stride, (hipStream_t)stream, IA_ENC_S);
}

extern "C" int ia_hash_desc_init(ia_hash_desc *o, int n_levels, int log2_hashmap_size, int base_resolution,
                                 float per_level_scale) {
  IA_CHECK_ARG(o && n_levels > 0 && n_levels <= IA_MAX_LEVELS, "ia_hash_desc_init: bad arguments");
  // tcnn grid.h: grid_scale(), grid_resolution(), GridEncodingTemplated ctor (host arithmetic)
  const float l2 = log2f(per_level_scale);
  uint32_t off = 0;
  o->n_levels = n_levels;
  for (int l = 0; l < n_levels; l++) {
    const float s = exp2f((float)l * l2) * (float)base_resolution - 1.0f;
    const uint32_t r = (uint32_t)ceilf(s) + 1;
    const uint32_t max_params = 0xffffffffu / 2;
    uint32_t n = powf((float)r, 3.f) > (float)max_params ? max_params : r * r * r;
    n = (n + 7u) / 8u * 8u;
    if (n > (1u << log2_hashmap_size)) n = 1u << log2_hashmap_size;
    o->scale[l] = s; o->res[l] = r; o->offset[l] = off;
    off += n;
  }
  o->offset[n_levels] = off;
  return IA_OK;
}
