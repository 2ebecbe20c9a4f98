// ia_smpl_dev.h -- device functions of the SMPL body model shared by ia_smpl_lbs.hip (single frame, T_inv) and ia_keypoints.hip
// (all frames, vertices and joints): Rodrigues and its backward, the 24-joint kinematic chain forward and reversed.
#pragma once
#include "ia_common.h"

// ---- Rodrigues (lbs.py:295-329): angle = |theta + 1e-8|, dir = theta / angle, R = I + sin K + (1 - cos) K^2 -----------
struct Rod { float ang, sn, cs, K[9], KK[9], R[9]; };
__device__ __forceinline__ void rodrigues(const float *th, Rod &r) {
  const float ax = th[0] + 1e-8f, ay = th[1] + 1e-8f, az = th[2] + 1e-8f;
  r.ang = sqrtf(ax * ax + ay * ay + az * az);
  const float d0 = th[0] / r.ang, d1 = th[1] / r.ang, d2 = th[2] / r.ang;
  r.cs = cosf(r.ang); r.sn = sinf(r.ang);
  const float k[9] = {0, -d2, d1, d2, 0, -d0, -d1, d0, 0};
  for (int a = 0; a < 9; a++) r.K[a] = k[a];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      float v = 0.f;
      for (int q = 0; q < 3; q++) v += r.K[a * 3 + q] * r.K[q * 3 + b];
      r.KK[a * 3 + b] = v;
    }
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) r.R[a * 3 + b] = (a == b ? 1.f : 0.f) + r.sn * r.K[a * 3 + b] + (1.f - r.cs) * r.KK[a * 3 + b];
}
__device__ __forceinline__ void rodrigues_bwd(const float *th, const Rod &r, const float *dR, float *dth) {
  float dK[9];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      float v = r.sn * dR[a * 3 + b];
      for (int q = 0; q < 3; q++) v += (1.f - r.cs) * (dR[a * 3 + q] * r.K[b * 3 + q] + r.K[q * 3 + a] * dR[q * 3 + b]);   // dR K^T + K^T dR
      dK[a * 3 + b] = v;
    }
  float dRK = 0.f, dRKK = 0.f;
  for (int a = 0; a < 9; a++) { dRK += dR[a] * r.K[a]; dRKK += dR[a] * r.KK[a]; }
  const float d_ang = r.cs * dRK + r.sn * dRKK;
  const float d_dir[3] = {dK[7] - dK[5], dK[2] - dK[6], dK[3] - dK[1]};
  const float dot = d_dir[0] * th[0] + d_dir[1] * th[1] + d_dir[2] * th[2];
  const float coef = d_ang - dot / (r.ang * r.ang);
  for (int a = 0; a < 3; a++) dth[a] = d_dir[a] / r.ang + coef * (th[a] + 1e-8f) / r.ang;
}

// One kinematic chain in LDS: L_j = [R_j | rel_j], G_0 = L_0, G_j = G_p L_j (lbs.py:345-401), sequentially over the joints with
// lane (a, b) of the first twelve owning one element.  R [24][9], Jn [24][3] -> G [24][12] (rows 0..2 of the 4x4).
__device__ __forceinline__ void chain_forward(const float (*R)[9], const float (*Jn)[3], const int *par, float (*G)[12], int j) {
  if (j < 12) {
    const int a = j >> 2, b = j & 3;
    G[0][j] = b < 3 ? R[0][a * 3 + b] : Jn[0][a];
  }
  __syncthreads();
  for (int i = 1; i < 24; i++) {
    if (j < 12) {
      const int a = j >> 2, b = j & 3, p = par[i];
      float acc;
      if (b < 3) acc = G[p][a * 4] * R[i][b] + G[p][a * 4 + 1] * R[i][3 + b] + G[p][a * 4 + 2] * R[i][6 + b];
      else acc = G[p][a * 4] * (Jn[i][0] - Jn[p][0]) + G[p][a * 4 + 1] * (Jn[i][1] - Jn[p][1]) + G[p][a * 4 + 2] * (Jn[i][2] - Jn[p][2]) + G[p][a * 4 + 3];
      G[i][j] = acc;
    }
    __syncthreads();
  }
}

// One chain reversed: d A_j (rows 0..2) (+ dGt: d of the translation of G_j, optional) -> d R_j (local rotations), d J accumulated.  dRG / dg are scratch [24][9] / [24][3].
// children before parents (parents[i] < i); lanes 0..8 own one element of the 3x3 products, lanes 9..11 the translation part.
__device__ __forceinline__ void chain_backward(const float (*dA)[12], const float (*R)[9], const float (*G)[12], const float (*Jn)[3],
                                               const int *par, float (*dRG)[9], float (*dg)[3], float (*dRl)[9], float (*dJ)[3], int j,
                                               const float (*dGt)[3] = nullptr) {
  if (j < 24) {
    for (int a = 0; a < 3; a++) {
      for (int b = 0; b < 3; b++) dRG[j][a * 3 + b] = dA[j][a * 4 + b] - dA[j][a * 4 + 3] * Jn[j][b];   // A.t = g - RG J (+ tau)
      float g = dA[j][a * 4 + 3];
      if (dGt) g += dGt[j][a];   // a caller's gradient of the posed joint itself (the translation of G_j)
      dg[j][a] = g;
    }
    for (int b = 0; b < 3; b++)    // d J_j -= RG_j^T dA_j.t
      dJ[j][b] -= G[j][b] * dA[j][3] + G[j][4 + b] * dA[j][7] + G[j][8 + b] * dA[j][11];
  }
  __syncthreads();
  for (int i = 23; i >= 1; i--) {
    const int p = par[i];
    if (j < 9) {
      const int a = j / 3, b = j - 3 * a;
      dRl[i][j] = G[p][a] * dRG[i][b] + G[p][4 + a] * dRG[i][3 + b] + G[p][8 + a] * dRG[i][6 + b];          // dR_i = RG_p^T dRG_i
      float wv = dg[i][a] * (Jn[i][b] - Jn[p][b]);                                                          // dg_i rel_i^T
      for (int q = 0; q < 3; q++) wv += dRG[i][a * 3 + q] * R[i][b * 3 + q];                                // + dRG_i R_i^T
      dRG[p][j] += wv;
    } else if (j < 12) {
      const int c = j - 9;
      const float drel = G[p][c] * dg[i][0] + G[p][4 + c] * dg[i][1] + G[p][8 + c] * dg[i][2];              // d rel_i = RG_p^T dg_i
      dJ[i][c] += drel;
      dJ[p][c] -= drel;
    }
    __syncthreads();
    if (j >= 9 && j < 12) dg[p][j - 9] += dg[i][j - 9];
    __syncthreads();
  }
  if (j < 9) dRl[0][j] = dRG[0][j];
  if (j < 3) dJ[0][j] += dg[0][j];     // rel_0 = J_0
  __syncthreads();
}
