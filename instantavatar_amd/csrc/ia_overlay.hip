// ia_overlay.hip -- the per-pixel work of looking at a custom sequence (include/instantavatar_hip_overlay.h; definitions in DESIGN.md
// section 4, "sequence inspection"): blend a shaded body layer into a batch of frames, draw the mask outline and the 2D skeleton into
// them, shade a face-id image flat, and count the pixels of two masks and of their intersection and union.  All of it is a gather per
// output pixel: nothing is scattered and no thread waits for another, so the bytes are a function of the inputs alone.
//
//   k_overlay_blend        a thread per 4 pixels: 12 image bytes as three dwords, 16 layer bytes as one dwordx4.  The batch is ONE run of
//                          n H W pixels, so rows of 3 W bytes need no care; what is ragged is the last 1..3 pixels of the batch, and a
//                          batch whose pointers are not aligned goes bytewise altogether
//   k_overlay_outline      a workgroup per 64 x 32 tile.  A wave ballots a row's "mask == 0 and inside the image" into a 64-bit word (its
//                          own columns and the two neighbouring words), ORs it with its shifts by 1..t (the row's zero pixels spread by t
//                          along x) and leaves the word in LDS; after the barrier an output row ORs the words of rows y - t .. y + t.
//                          Only outline pixels are stored
//   k_overlay_face_shade   a thread per pixel
//   k_overlay_skeleton     a wave per 32 x 16 tile.  Lane k quantises point k, lane s looks segment s up; both test their primitive's
//                          bounding box, grown by the disc radius or the half width, against the tile, and the two ballots are the tile's
//                          survivors.  A tile without survivors ends there (most of a 1080p frame); the others walk the survivor bits per
//                          pixel.  Loops: at most 64 + 64 survivors, 8 pixels per lane
//   k_overlay_stats_*      16 bytes of either mask per lane and step, non-zero bytes counted by popcount; partial sums per workgroup, then
//                          a wave per frame
//
// The skeleton's one product that can pass 64 bits is the square of the cross product c = d_x e_y - d_y e_x (|c| < 2^38) against
// hw^2 L2 < 2^50.  It is compared exactly without a 128-bit multiply: |c| >= 2^32 means c^2 >= 2^64 > hw^2 L2, so the pixel is outside;
// below that c^2 fits 64 bits.
#include "ia_common.h"
#include "../../include/instantavatar_hip_overlay.h"

namespace {

typedef unsigned long long u64;

// ---- ia_overlay_blend -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ov_mix(uint32_t img, uint32_t lay, uint32_t a) { return (img * (256u - a) + lay * a + 128u) >> 8; }
__device__ __forceinline__ uint32_t ov_alpha(int opacity, uint32_t A) { return ((uint32_t)opacity * A + 127u) / 255u; }

__global__ __launch_bounds__(256) void k_overlay_blend(const uint8_t *images, const uint8_t *__restrict__ layer, size_t n_px, int opacity,
                                                       int wide, uint8_t *out) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, p0 = g * 4;
  if (p0 >= n_px) return;
  if (wide && p0 + 4 <= n_px) {
    const uint4 L = ((const uint4 *)layer)[g];
    const uint32_t *s = (const uint32_t *)images + g * 3;
    const uint32_t in[3] = {s[0], s[1], s[2]}, lw[4] = {L.x, L.y, L.z, L.w};
    uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t a = ov_alpha(opacity, lw[k] >> 24);
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int byte = 3 * k + c;          // of the 12: pixel k, channel c
        o[byte >> 2] |= ov_mix((in[byte >> 2] >> (8 * (byte & 3))) & 255u, (lw[k] >> (8 * c)) & 255u, a) << (8 * (byte & 3));
      }
    }
    uint32_t *d = (uint32_t *)out + g * 3;
    d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
    return;
  }
  for (size_t p = p0; p < n_px && p < p0 + 4; p++) {
    const uint32_t a = ov_alpha(opacity, layer[p * 4 + 3]);
    const uint32_t r = ov_mix(images[p * 3], layer[p * 4], a), gg = ov_mix(images[p * 3 + 1], layer[p * 4 + 1], a),
                   bb = ov_mix(images[p * 3 + 2], layer[p * 4 + 2], a);
    out[p * 3] = (uint8_t)r; out[p * 3 + 1] = (uint8_t)gg; out[p * 3 + 2] = (uint8_t)bb;
  }
}

// ---- ia_overlay_outline ---------------------------------------------------------------------------------------------------------------
#define OV_OL_ROWS 32

__global__ __launch_bounds__(256) void k_overlay_outline(const uint8_t *__restrict__ masks, int H, int W, int t, int r, int g, int b,
                                                         uint8_t *images) {
  __shared__ u64 s_zero[OV_OL_ROWS + 2 * IA_OVERLAY_MAX_THICKNESS], s_on[OV_OL_ROWS + 2 * IA_OVERLAY_MAX_THICKNESS];
  const int f = blockIdx.z, x0 = blockIdx.x * 64, y0 = blockIdx.y * OV_OL_ROWS;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint8_t *fr = masks + (size_t)f * H * W;
  const int rows = OV_OL_ROWS + 2 * t;                         // image rows y0 - t .. y0 + 31 + t
  for (int i = wave; i < rows; i += 4) {
    const int y = y0 - t + i;
    u64 zero = 0ull, on = 0ull;                                // a row outside the image holds no zero pixel that counts
    if (y >= 0 && y < H) {
      const uint8_t *row = fr + (size_t)y * W;
      const int xc = x0 + lane, xl = xc - 64, xr = xc + 64;
      const int vc = xc < W ? row[xc] : 255, vl = xl >= 0 ? row[xl] : 255, vr = xr < W ? row[xr] : 255;      // outside: not a zero pixel
      const u64 zc = __ballot(vc == 0), zl = __ballot(vl == 0), zr = __ballot(vr == 0);
      on = __ballot(xc < W && vc > 0);
      zero = zc;
      for (int d = 1; d <= t; d++) zero |= (zc >> d) | (zr << (64 - d)) | (zc << d) | (zl >> (64 - d));      // pixels x + d and x - d
    }
    if (lane == 0) { s_zero[i] = zero; s_on[i] = on; }
  }
  __syncthreads();
  for (int ry = wave; ry < OV_OL_ROWS; ry += 4) {
    const int y = y0 + ry;
    if (y >= H) break;
    u64 near = 0ull;
    for (int d = 0; d <= 2 * t; d++) near |= s_zero[ry + d];   // rows y - t .. y + t
    if (((near & s_on[ry + t]) >> lane) & 1ull) {
      uint8_t *p = images + (((size_t)f * H + y) * W + x0 + lane) * 3;
      p[0] = (uint8_t)r; p[1] = (uint8_t)g; p[2] = (uint8_t)b;
    }
  }
}

// ---- ia_overlay_face_shade ------------------------------------------------------------------------------------------------------------
struct OvRot { float m[9]; };

__global__ __launch_bounds__(256) void k_overlay_face_shade(const int32_t *__restrict__ face_id, int n_px, const float *__restrict__ verts,
                                                            int nv, const int32_t *__restrict__ faces, int nf,
                                                            const float *__restrict__ w2c, float tr, float tg, float tb,
                                                            uint32_t *__restrict__ layer) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_px) return;
  const int fid = face_id[p];
  uint32_t px = 0u;
  if (fid >= 0 && fid < nf) {
    const int i0 = faces[3 * fid], i1 = faces[3 * fid + 1], i2 = faces[3 * fid + 2];
    if (i0 >= 0 && i0 < nv && i1 >= 0 && i1 < nv && i2 >= 0 && i2 < nv) {
      const float *v0 = verts + 3 * (size_t)i0, *v1 = verts + 3 * (size_t)i1, *v2 = verts + 3 * (size_t)i2;
      const float ax = v1[0] - v0[0], ay = v1[1] - v0[1], az = v1[2] - v0[2], bx = v2[0] - v0[0], by = v2[1] - v0[1], bz = v2[2] - v0[2];
      float d1[3], d2[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {      // the rotation block of the row-major [4,4]
        d1[k] = w2c[4 * k] * ax + w2c[4 * k + 1] * ay + w2c[4 * k + 2] * az;
        d2[k] = w2c[4 * k] * bx + w2c[4 * k + 1] * by + w2c[4 * k + 2] * bz;
      }
      const float cx = d1[1] * d2[2] - d1[2] * d2[1], cy = d1[2] * d2[0] - d1[0] * d2[2], cz = d1[0] * d2[1] - d1[1] * d2[0];
      const float len = sqrtf(cx * cx + cy * cy + cz * cz);
      float s = 0.25f;
      if (len > 0.f && len <= 3.0e38f) s = 0.25f + 0.75f * (fabsf(cz) / len);      // (false for NaN and inf as well)
      const uint32_t rr = (uint32_t)floorf(tr * s + 0.5f), gg = (uint32_t)floorf(tg * s + 0.5f), bb = (uint32_t)floorf(tb * s + 0.5f);
      px = rr | (gg << 8) | (bb << 16) | 0xff000000u;
    }
  }
  layer[p] = px;
}

// ---- ia_overlay_skeleton --------------------------------------------------------------------------------------------------------------
#define OV_SK_W 32
#define OV_SK_H 16

__global__ __launch_bounds__(64) void k_overlay_skeleton(const float *__restrict__ points, int K, const int32_t *__restrict__ segments,
                                                         const uint8_t *__restrict__ segment_rgb, int S, int pr, int pg, int pb,
                                                         float threshold, int hw, int rad, int H, int W, uint8_t *images) {
  __shared__ int s_qx[64], s_qy[64], s_seg[64][4];
  __shared__ uint32_t s_rgb[64];
  const int f = blockIdx.z, lane = threadIdx.x;
  const int tx0 = blockIdx.x * OV_SK_W, ty0 = blockIdx.y * OV_SK_H;
  const int tx1 = (tx0 + OV_SK_W < W ? tx0 + OV_SK_W : W) - 1, ty1 = (ty0 + OV_SK_H < H ? ty0 + OV_SK_H : H) - 1;
  const int cx0 = 4 * tx0, cx1 = 4 * tx1, cy0 = 4 * ty0, cy1 = 4 * ty1;      // the tile's pixel centres, in quarter pixels
  bool valid = false;
  int qx = 0, qy = 0;
  if (lane < K) {
    const float *p = points + ((size_t)f * K + lane) * 3;
    const float x = p[0], y = p[1], c = p[2];
    valid = fabsf(x) <= 32768.f && fabsf(y) <= 32768.f && fabsf(c) <= 3.4028234664e38f && c > threshold;      // NaN and inf fail a <=
    if (valid) { qx = (int)floorf(4.f * x + 0.5f); qy = (int)floorf(4.f * y + 0.5f); }
  }
  s_qx[lane] = qx; s_qy[lane] = qy;
  const u64 vmask = __ballot(valid);
  const u64 discs = __ballot(valid && qx + rad >= cx0 && qx - rad <= cx1 && qy + rad >= cy0 && qy - rad <= cy1);
  __syncthreads();
  bool hit = false;
  if (lane < S) {
    const int i = segments[2 * lane], j = segments[2 * lane + 1];
    if (i >= 0 && i < K && j >= 0 && j < K && ((vmask >> i) & 1ull) && ((vmask >> j) & 1ull)) {
      const int ax = s_qx[i], ay = s_qy[i], bx = s_qx[j], by = s_qy[j];
      const int lox = (ax < bx ? ax : bx) - hw, hix = (ax < bx ? bx : ax) + hw, loy = (ay < by ? ay : by) - hw, hiy = (ay < by ? by : ay) + hw;
      hit = hix >= cx0 && lox <= cx1 && hiy >= cy0 && loy <= cy1;
      if (hit) {
        s_seg[lane][0] = ax; s_seg[lane][1] = ay; s_seg[lane][2] = bx; s_seg[lane][3] = by;
        s_rgb[lane] = (uint32_t)segment_rgb[3 * lane] | ((uint32_t)segment_rgb[3 * lane + 1] << 8) | ((uint32_t)segment_rgb[3 * lane + 2] << 16);
      }
    }
  }
  const u64 segs = __ballot(hit);
  if (!(discs | segs)) return;      // wave-uniform: nothing of this frame comes near the tile
  __syncthreads();
  const long long hw2 = (long long)hw * hw, rad2 = (long long)rad * rad;
  const int px = tx0 + (lane & 31);
  for (int r = 0; r < OV_SK_H / 2; r++) {
    const int py = ty0 + (lane >> 5) + 2 * r;
    if (px > tx1 || py > ty1) continue;
    const int X = 4 * px, Y = 4 * py;
    bool disc = false;
    for (u64 m = discs; m; m &= m - 1) {
      const int k = __ffsll((long long)m) - 1;
      const long long dx = X - s_qx[k], dy = Y - s_qy[k];
      disc |= dx * dx + dy * dy <= rad2;
    }
    int top = -1;                                             // ascending: the highest covering index is the last one kept
    for (u64 m = disc ? 0ull : segs; m; m &= m - 1) {
      const int k = __ffsll((long long)m) - 1;
      const int ax = s_seg[k][0], ay = s_seg[k][1], bx = s_seg[k][2], by = s_seg[k][3];
      const long long dx = bx - ax, dy = by - ay, ex = X - ax, ey = Y - ay;
      const long long L2 = dx * dx + dy * dy, t = dx * ex + dy * ey;
      bool in;
      if (L2 == 0 || t <= 0) in = ex * ex + ey * ey <= hw2;
      else if (t >= L2) { const long long fx = X - bx, fy = Y - by; in = fx * fx + fy * fy <= hw2; }
      else {
        const long long c = dx * ey - dy * ex;
        const u64 ac = (u64)(c < 0 ? -c : c);
        in = ac < (1ull << 32) && ac * ac <= (u64)hw2 * (u64)L2;      // exact: see the head of the file
      }
      if (in) top = k;
    }
    if (!disc && top < 0) continue;
    const uint32_t col = disc ? ((uint32_t)pr | ((uint32_t)pg << 8) | ((uint32_t)pb << 16)) : s_rgb[top];
    uint8_t *o = images + (((size_t)f * H + py) * W + px) * 3;
    o[0] = (uint8_t)(col & 255u); o[1] = (uint8_t)((col >> 8) & 255u); o[2] = (uint8_t)((col >> 16) & 255u);
  }
}

// ---- ia_overlay_stats -----------------------------------------------------------------------------------------------------------------
// high bit of every non-zero byte of w
__device__ __forceinline__ uint32_t ov_nonzero(uint32_t w) { return (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u; }

__device__ __forceinline__ void ov_count(uint32_t x, uint32_t y, int *c) {
  const uint32_t ma = ov_nonzero(x), mb = ov_nonzero(y);
  c[0] += __popc(ma & mb); c[1] += __popc(ma | mb); c[2] += __popc(ma); c[3] += __popc(mb);
}

// blocks per frame: a block takes 64 KiB of either mask per turn
int stats_blocks(long long hw) {
  const long long b = (hw + 65535) / 65536;
  return (int)(b < 1 ? 1 : b > 256 ? 256 : b);
}

__global__ __launch_bounds__(256) void k_overlay_stats_partial(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, int HW, int B,
                                                               int wide, int32_t *__restrict__ partial) {
  __shared__ int s_c[4][4];
  const int f = blockIdx.y, blk = blockIdx.x;
  const uint8_t *fa = a + (size_t)f * HW, *fb = b + (size_t)f * HW;
  int c[4] = {0, 0, 0, 0};
  // wide: both frames start at the same offset within 16 bytes.  [0, head) bytewise, then `units` 16-byte pieces, then the rest bytewise
  int head = 0, units = 0;
  if (wide) {
    head = (int)((16u - (uint32_t)((uintptr_t)fa & 15u)) & 15u);
    if (head > HW) head = HW;
    units = (HW - head) / 16;
  }
  const uint4 *va = (const uint4 *)(fa + head), *vb = (const uint4 *)(fb + head);
  for (int u = blk * 256 + (int)threadIdx.x; u < units; u += B * 256) {      // u < 2^27, B * 256 <= 2^16
    const uint4 x = va[u], y = vb[u];
    ov_count(x.x, y.x, c); ov_count(x.y, y.y, c); ov_count(x.z, y.z, c); ov_count(x.w, y.w, c);
  }
  const int body_end = head + 16 * units, left = head + (HW - body_end);     // bytes outside the 16-byte pieces (all of them when !wide)
  for (long long i = (long long)blk * 256 + threadIdx.x; i < left; i += (long long)B * 256) {
    const int p = i < head ? (int)i : body_end + (int)(i - head);
    const bool A = fa[p] != 0, Bb = fb[p] != 0;
    c[0] += A && Bb; c[1] += A || Bb; c[2] += A; c[3] += Bb;
  }
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_xor(c[k], o, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { s_c[wave][0] = c[0]; s_c[wave][1] = c[1]; s_c[wave][2] = c[2]; s_c[wave][3] = c[3]; }
  __syncthreads();
  if (threadIdx.x < 4) partial[((size_t)f * B + blk) * 4 + threadIdx.x] = s_c[0][threadIdx.x] + s_c[1][threadIdx.x] + s_c[2][threadIdx.x] + s_c[3][threadIdx.x];
}

__global__ __launch_bounds__(64) void k_overlay_stats_final(const int32_t *__restrict__ partial, int B, int32_t *__restrict__ out) {
  const int f = blockIdx.x, lane = threadIdx.x;
  int c[4] = {0, 0, 0, 0};
  for (int i = lane; i < B; i += 64) {
    const int32_t *p = partial + ((size_t)f * B + i) * 4;
    c[0] += p[0]; c[1] += p[1]; c[2] += p[2]; c[3] += p[3];
  }
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_xor(c[k], o, 64);
  if (lane < 4) out[(size_t)f * 4 + lane] = lane == 0 ? c[0] : lane == 1 ? c[1] : lane == 2 ? c[2] : c[3];
}

bool overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && x < y + nb && y < x + na;
}

bool frames_ok(int n, int H, int W) { return n >= 1 && n <= IA_OVERLAY_MAX_FRAMES && H >= 1 && W >= 1 && (long long)H * W < (1ll << 31); }
bool colour_ok(int r, int g, int b) { return r >= 0 && r <= 255 && g >= 0 && g <= 255 && b >= 0 && b <= 255; }

}  // namespace

extern "C" int ia_overlay_blend(const uint8_t *images, const uint8_t *layer, int n, int H, int W, int opacity, uint8_t *out, void *stream) {
  IA_CHECK_ARG(stream != nullptr, "ia_overlay_blend: an explicit stream is required (stream = NULL)");
  IA_CHECK_ARG(frames_ok(n, H, W), "ia_overlay_blend: %d frames of %d x %d: outside 1 <= n <= %d, H, W >= 1, H * W < 2^31", n, H, W,
               IA_OVERLAY_MAX_FRAMES);
  IA_CHECK_ARG(opacity >= 0 && opacity <= 256, "ia_overlay_blend: opacity %d outside [0, 256]", opacity);
  IA_CHECK_ARG(images && layer && out, "ia_overlay_blend: images, layer and out are required");
  const size_t px = (size_t)n * H * W;
  IA_CHECK_ARG(px / 4 / 256 < (size_t)INT_MAX, "ia_overlay_blend: %zu pixels are too many for one launch", px);
  IA_CHECK_ARG(out == images || !overlap(images, px * 3, out, px * 3), "ia_overlay_blend: out may be images itself, not overlap it otherwise");
  IA_CHECK_ARG(!overlap(layer, px * 4, out, px * 3), "ia_overlay_blend: out overlaps layer");
  const int wide = (((uintptr_t)images | (uintptr_t)out) & 3) == 0 && ((uintptr_t)layer & 15) == 0;
  hipLaunchKernelGGL(k_overlay_blend, dim3(ia_div_up((long)((px + 3) / 4), 256)), dim3(256), 0, (hipStream_t)stream, images, layer, px, opacity,
                     wide, out);
  IA_LAUNCH_CHECK("k_overlay_blend");
  return IA_OK;
}

extern "C" int ia_overlay_outline(const uint8_t *masks, int n, int H, int W, int thickness, int r, int g, int b, uint8_t *images,
                                  void *stream) {
  IA_CHECK_ARG(stream != nullptr, "ia_overlay_outline: an explicit stream is required (stream = NULL)");
  IA_CHECK_ARG(frames_ok(n, H, W), "ia_overlay_outline: %d frames of %d x %d: outside 1 <= n <= %d, H, W >= 1, H * W < 2^31", n, H, W,
               IA_OVERLAY_MAX_FRAMES);
  IA_CHECK_ARG(thickness >= 1 && thickness <= IA_OVERLAY_MAX_THICKNESS, "ia_overlay_outline: thickness %d outside [1, %d]", thickness,
               IA_OVERLAY_MAX_THICKNESS);
  IA_CHECK_ARG(colour_ok(r, g, b), "ia_overlay_outline: colour (%d, %d, %d) outside [0, 255]", r, g, b);
  IA_CHECK_ARG(masks && images, "ia_overlay_outline: masks and images are required");
  const size_t px = (size_t)n * H * W;
  IA_CHECK_ARG(!overlap(masks, px, images, px * 3), "ia_overlay_outline: images overlaps masks");
  IA_CHECK_ARG(ia_div_up(H, OV_OL_ROWS) <= 65535, "ia_overlay_outline: H = %d is too tall for one launch", H);
  hipLaunchKernelGGL(k_overlay_outline, dim3(ia_div_up(W, 64), ia_div_up(H, OV_OL_ROWS), n), dim3(256), 0, (hipStream_t)stream, masks, H, W,
                     thickness, r, g, b, images);
  IA_LAUNCH_CHECK("k_overlay_outline");
  return IA_OK;
}

extern "C" int ia_overlay_face_shade(const int32_t *face_id, int H, int W, const float *verts, int nv, const int32_t *faces, int nf,
                                     const float *w2c, int r, int g, int b, uint8_t *layer, void *stream) {
  IA_CHECK_ARG(stream != nullptr, "ia_overlay_face_shade: an explicit stream is required (stream = NULL)");
  IA_CHECK_ARG(frames_ok(1, H, W), "ia_overlay_face_shade: a %d x %d image: outside H, W >= 1, H * W < 2^31", H, W);
  IA_CHECK_ARG(nv >= 1 && nf >= 1 && nv <= INT_MAX / 3 && nf <= INT_MAX / 3, "ia_overlay_face_shade: %d vertices and %d faces: at least one of each",
               nv, nf);
  IA_CHECK_ARG(colour_ok(r, g, b), "ia_overlay_face_shade: tint (%d, %d, %d) outside [0, 255]", r, g, b);
  IA_CHECK_ARG(face_id && verts && faces && w2c && layer, "ia_overlay_face_shade: face_id, verts, faces, w2c and layer are required");
  IA_CHECK_ARG((((uintptr_t)face_id | (uintptr_t)verts | (uintptr_t)faces | (uintptr_t)w2c | (uintptr_t)layer) & 3) == 0,
               "ia_overlay_face_shade: face_id, verts, faces, w2c and layer must be 4-byte aligned");
  const size_t px = (size_t)H * W;
  IA_CHECK_ARG(!overlap(face_id, px * 4, layer, px * 4), "ia_overlay_face_shade: layer overlaps face_id");
  hipLaunchKernelGGL(k_overlay_face_shade, dim3(ia_div_up((long)px, 256)), dim3(256), 0, (hipStream_t)stream, face_id, (int)px, verts, nv, faces,
                     nf, w2c, (float)r, (float)g, (float)b, (uint32_t *)layer);
  IA_LAUNCH_CHECK("k_overlay_face_shade");
  return IA_OK;
}

extern "C" int ia_overlay_skeleton(const float *points, int n, int K, const int32_t *segments, const uint8_t *segment_rgb, int S, int point_r,
                                   int point_g, int point_b, float threshold, int half_width_q, int radius_q, int H, int W, uint8_t *images,
                                   void *stream) {
  IA_CHECK_ARG(stream != nullptr, "ia_overlay_skeleton: an explicit stream is required (stream = NULL)");
  IA_CHECK_ARG(frames_ok(n, H, W) && H <= 32768 && W <= 32768,
               "ia_overlay_skeleton: %d frames of %d x %d: outside 1 <= n <= %d, 1 <= H, W <= 32768, H * W < 2^31", n, H, W, IA_OVERLAY_MAX_FRAMES);
  IA_CHECK_ARG(K >= 1 && K <= IA_OVERLAY_MAX_POINTS, "ia_overlay_skeleton: K = %d points outside [1, %d]", K, IA_OVERLAY_MAX_POINTS);
  IA_CHECK_ARG(S >= 0 && S <= IA_OVERLAY_MAX_SEGMENTS, "ia_overlay_skeleton: S = %d segments outside [0, %d]", S, IA_OVERLAY_MAX_SEGMENTS);
  IA_CHECK_ARG(half_width_q >= 1 && half_width_q <= 64, "ia_overlay_skeleton: half_width_q %d outside [1, 64] (quarter pixels)", half_width_q);
  IA_CHECK_ARG(radius_q >= 0 && radius_q <= 128, "ia_overlay_skeleton: radius_q %d outside [0, 128] (quarter pixels)", radius_q);
  IA_CHECK_ARG(colour_ok(point_r, point_g, point_b), "ia_overlay_skeleton: point colour (%d, %d, %d) outside [0, 255]", point_r, point_g, point_b);
  IA_CHECK_ARG(threshold == threshold, "ia_overlay_skeleton: threshold is NaN");
  IA_CHECK_ARG(points && images && (S == 0 || (segments && segment_rgb)), "ia_overlay_skeleton: points and images are required, and segments and segment_rgb when S > 0");
  IA_CHECK_ARG((((uintptr_t)points | (uintptr_t)segments) & 3) == 0, "ia_overlay_skeleton: points and segments must be 4-byte aligned");
  hipLaunchKernelGGL(k_overlay_skeleton, dim3(ia_div_up(W, OV_SK_W), ia_div_up(H, OV_SK_H), n), dim3(64), 0, (hipStream_t)stream, points, K,
                     segments, segment_rgb, S, point_r, point_g, point_b, threshold, half_width_q, radius_q, H, W, images);
  IA_LAUNCH_CHECK("k_overlay_skeleton");
  return IA_OK;
}

extern "C" size_t ia_overlay_stats_workspace_bytes(int n, int H, int W) {
  if (!frames_ok(n, H, W)) return 0;
  return ia_align((size_t)n * stats_blocks((long long)H * W) * 4 * sizeof(int32_t));
}

extern "C" int ia_overlay_stats(const uint8_t *a, const uint8_t *b, int n, int H, int W, int32_t *out, void *ws, size_t ws_bytes,
                                void *stream) {
  IA_CHECK_ARG(stream != nullptr, "ia_overlay_stats: an explicit stream is required (stream = NULL)");
  IA_CHECK_ARG(frames_ok(n, H, W), "ia_overlay_stats: %d frames of %d x %d: outside 1 <= n <= %d, H, W >= 1, H * W < 2^31", n, H, W,
               IA_OVERLAY_MAX_FRAMES);
  IA_CHECK_ARG(a && b && out, "ia_overlay_stats: a, b and out are required");
  const size_t need = ia_overlay_stats_workspace_bytes(n, H, W);
  IA_CHECK_ARG(ws && ws_bytes >= need, "ia_overlay_stats: workspace of %zu bytes, %zu needed (ia_overlay_stats_workspace_bytes)",
               ws ? ws_bytes : (size_t)0, need);
  IA_CHECK_ARG(((uintptr_t)ws & 3) == 0 && ((uintptr_t)out & 3) == 0, "ia_overlay_stats: ws and out must be 4-byte aligned");
  const size_t px = (size_t)n * H * W;
  IA_CHECK_ARG(!overlap(a, px, out, (size_t)n * 16) && !overlap(b, px, out, (size_t)n * 16), "ia_overlay_stats: out overlaps a mask");
  const int HW = H * W, B = stats_blocks(HW);
  const int wide = (((uintptr_t)a ^ (uintptr_t)b) & 15) == 0;
  hipLaunchKernelGGL(k_overlay_stats_partial, dim3(B, n), dim3(256), 0, (hipStream_t)stream, a, b, HW, B, wide, (int32_t *)ws);
  hipLaunchKernelGGL(k_overlay_stats_final, dim3(n), dim3(64), 0, (hipStream_t)stream, (const int32_t *)ws, B, out);
  IA_LAUNCH_CHECK("k_overlay_stats");
  return IA_OK;
}
