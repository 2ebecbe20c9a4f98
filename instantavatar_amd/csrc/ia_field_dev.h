// ia_field_dev.h -- device vocabulary of the canonical field shared by ia_field.hip (forward, backward, encoder) and
// ia_normals.hip (k_sigma_grad): MFMA vector types, the A-fragment table of the two MLPs, the normalisation of a sample
// position and the tcnn cell / corner arithmetic of one hash-grid level.  Definitions only; the work decomposition they serve
// is described in ia_field.hip's file header.
#pragma once
#include "ia_common.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0)

#define N_FRAG 22
#define F_SIG1 0   // [rb(2)][s(2)]
#define F_SIG2 4   // [s(4)]
#define F_COL1 8   // [rb(2)]
#define F_COL2 10  // [rb(2)][s(4)]
#define F_COL3 18  // [s(4)]

__device__ __forceinline__ _Float16 ld_h(const uint16_t *w, int idx) {
  union { uint16_t u; _Float16 h; } c;
  c.u = w[idx];
  return c.h;
}

// Weight value of A-fragment f at lane (i = out row in its 32-block, h) and
// position p (0..7).  k-permutations explained in ia_field.hip's file header.
template <int L>
__device__ _Float16 frag_value(const FieldDev &F, int f, int i, int h, int p) {
  const int kk = (p & 3) + 8 * (p >> 2) + 4 * h;  // C/D row order inside a 16-row slab
  if (f < F_SIG2) {
    const int rb = f >> 1, s = f & 1;
    if (s >= L / 8) return (_Float16)0.f;
    return ld_h(F.sig_w1, (rb * 32 + i) * (2 * L) + h * L + 8 * s + p);
  }
  if (f < F_COL1) {
    const int s = f - F_SIG2;
    return i < 16 ? ld_h(F.sig_w2, i * 64 + 16 * s + kk) : (_Float16)0.f;
  }
  if (f < F_COL2) {
    // colour input c[m] = out[m+1] (m < 15), c[15] = 1 (tcnn identity padding);
    // our B slot kk holds out[kk] for kk >= 1 and the constant 1 at kk == 0.
    const int rb = f - F_COL1;
    return ld_h(F.col_w1, (rb * 32 + i) * 16 + (kk == 0 ? 15 : kk - 1));
  }
  if (f < F_COL3) {
    const int rb = (f - F_COL2) >> 2, s = (f - F_COL2) & 3;
    return ld_h(F.col_w2, (rb * 32 + i) * 64 + 16 * s + kk);
  }
  const int s = f - F_COL3;
  return i < 16 ? ld_h(F.col_w3, i * 64 + 16 * s + kk) : (_Float16)0.f;
}

__device__ __forceinline__ void normalise(const FieldDev &F, const float *__restrict__ x, size_t i,
                                          float xn[3]) {
#pragma unroll
  for (int d = 0; d < 3; d++) {
    float v = (x[i * 3 + d] - F.center[d]) / F.scale[d] + 0.5f;  // ngp.py:75
    v = v < 0.f ? 0.f : v;                                       // ngp.py:77 clamp
    v = v > 1.f ? 1.f : v;
    xn[d] = v;
  }
}

template <bool RELU>
__device__ __forceinline__ half8 pack_slab(const floatx16 &acc, int sub) {
  half8 o;
#pragma unroll
  for (int p = 0; p < 8; p++) {
    float v = acc[8 * sub + p];
    if (RELU) v = v < 0.f ? 0.f : v;
    o[p] = (_Float16)v;
  }
  return o;
}

// C/D row of accumulator register r in lane half h (inside a 32-row block)
__device__ __forceinline__ int cd_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// tcnn pos_fract: cell g and fractional position w of a normalised sample position at one level
__device__ __forceinline__ void pos_fract(const float xn[3], float scale, uint32_t g[3], float w[3]) {
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const float pos = __builtin_fmaf(xn[d], scale, 0.5f);  // nvcc contracts tcnn's `input * scale + 0.5f`
    const float fl = floorf(pos);
    g[d] = (uint32_t)(int)fl;
    w[d] = pos - fl;
  }
}

// tcnn grid_index: table entry of corner (cx, cy, cz) -- coherent prime hash (2^k entries) or dense index
__device__ __forceinline__ uint32_t corner_index(bool hashed, uint32_t cx, uint32_t cy, uint32_t cz, uint32_t res, uint32_t size) {
  if (hashed) return (cx ^ (cy * 2654435761u) ^ (cz * 805459861u)) & (size - 1);
  uint32_t index = cx + cy * res + cz * res * res;  // < 2*size for clamped inputs (tcnn: index % size)
  if (index >= size) index -= size;
  return min(index, size - 1);  // memory safety for non-finite inputs
}
