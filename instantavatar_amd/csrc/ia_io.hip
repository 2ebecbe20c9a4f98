// ia_io.hip -- sequence ingest: decoded full-resolution frames -> the resident stores of datasets.DeviceFrames.
//
// Reference semantics: instant_avatar/datasets/peoplesnapshot.py:100-107 and custom.py:98-105 -- per item, on the host,
// cv2.resize(img / msk, fx = fy = 1 / downscale) followed by astype(float32) of the mask.  Here once per sequence, one
// launch per staged chunk of frames, writing frame i of the images / masks stores in place.
//
// The resize rule (include/instantavatar_hip_io.h): for fx = fy = 0.5 OpenCV's own dispatch replaces INTER_LINEAR by
// INTER_AREA (both integer scales are exactly 2), the rounded 2 x 2 box (a + b + c + d + 2) >> 2 for uint8 sources and the
// plain float64 mean for the custom layout's float64 mask.  Other factors and odd source sizes would go through OpenCV's
// fixed-point bilinear path and its edge handling, which are not restated: they are refused, not approximated.
//
// Memory access: a lane takes 8 output pixels of one output row (factor 2: 2 x 48 source bytes of an image, 2 x 16 of a
// mask) or 16 bytes of a frame (factor 1), with 16-byte loads / the widest stores where the addresses allow it -- a
// source row of W0 * 3 bytes is not a multiple of 16 in general (1080 * 3 = 3240), so the tier is chosen per row -- and
// the last lane of a row takes the pixels that do not fill a group, one by one.
#include "ia_common.h"
#include "../../include/instantavatar_hip_io.h"

namespace {

// NW 32-bit words (a multiple of 4) starting at p, little endian, with the widest loads p's alignment allows
template <int NW> __device__ __forceinline__ void io_load(const uint8_t *__restrict__ p, uint32_t (&w)[NW]) {
  const uintptr_t a = (uintptr_t)p;
  if ((a & 15) == 0) {
#pragma unroll
    for (int i = 0; i < NW / 4; i++) {
      const uint4 v = ((const uint4 *)p)[i];
      w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
  } else if ((a & 3) == 0) {
#pragma unroll
    for (int i = 0; i < NW; i++) w[i] = ((const uint32_t *)p)[i];
  } else {
#pragma unroll
    for (int i = 0; i < NW; i++)
      w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
  }
}

template <int NW> __device__ __forceinline__ void io_store(uint8_t *__restrict__ q, const uint32_t (&w)[NW]) {
  const uintptr_t a = (uintptr_t)q;
  if (NW % 4 == 0 && (a & 15) == 0) {
#pragma unroll
    for (int i = 0; i < NW / 4; i++) ((uint4 *)q)[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
  } else if (NW % 2 == 0 && (a & 7) == 0) {
#pragma unroll
    for (int i = 0; i < NW / 2; i++) ((uint2 *)q)[i] = make_uint2(w[2 * i], w[2 * i + 1]);
  } else if ((a & 3) == 0) {
#pragma unroll
    for (int i = 0; i < NW; i++) ((uint32_t *)q)[i] = w[i];
  } else {
#pragma unroll
    for (int i = 0; i < NW * 4; i++) q[i] = (uint8_t)(w[i >> 2] >> ((i & 3) * 8));
  }
}

template <int NF> __device__ __forceinline__ void io_store_f(float *__restrict__ q, const float (&f)[NF]) {
  if (((uintptr_t)q & 15) == 0) {
#pragma unroll
    for (int i = 0; i < NF / 4; i++) ((float4 *)q)[i] = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
  } else {
#pragma unroll
    for (int i = 0; i < NF; i++) q[i] = f[i];
  }
}

template <int NW> __device__ __forceinline__ uint32_t io_byte(const uint32_t (&w)[NW], int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 255u; }

__device__ __forceinline__ uint32_t io_box_u8(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return (a + b + c + d + 2u) >> 2; }

// a mask pixel at factor 1: msk.astype(float32) of the uint8 array, or of the float64 array v / 255
__device__ __forceinline__ float io_mask1(uint32_t v, int form) {
  return form == IA_IO_MASK_GREY ? (float)((double)v / 255.0) : (float)v;
}

// a mask pixel at factor 2 (a b: upper row, c d: lower row)
__device__ __forceinline__ float io_mask4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, int form) {
  if (form == IA_IO_MASK_GREY) {
    const double up = (double)a / 255.0 + (double)b / 255.0, lo = (double)c / 255.0 + (double)d / 255.0;
    return (float)((up + lo) * 0.25);
  }
  return (float)io_box_u8(a, b, c, d);
}

// grid: x = work units of a frame's plane (groups of a row / of the frame, plus one tail unit per row / frame),
//       y = plane (0: image, 1: mask), z = frame of the chunk
__global__ __launch_bounds__(256) void k_io_ingest(const uint8_t *__restrict__ src_img, const uint8_t *__restrict__ src_msk, int form,
                                                   int H0, int W0, int factor, uint8_t *__restrict__ images,
                                                   float *__restrict__ masks, long long first) {
  const int f = blockIdx.z;
  const int u = blockIdx.x * 256 + threadIdx.x;
  const int H = H0 / factor, W = W0 / factor;
  const size_t src_px = (size_t)H0 * W0, dst_px = (size_t)H * W;
  if (blockIdx.y == 0) {
    if (!src_img) return;
    const uint8_t *s = src_img + (size_t)f * src_px * 3;
    uint8_t *d = images + ((size_t)first + f) * dst_px * 3;
    if (factor == 1) {
      const int nb = H0 * W0 * 3, ng = nb / 16;
      if (u < ng) {
        uint32_t w[4];
        io_load(s + (size_t)u * 16, w);
        io_store(d + (size_t)u * 16, w);
      } else if (u == ng) {
        for (int k = ng * 16; k < nb; k++) d[k] = s[k];
      }
      return;
    }
    const int ng = W / 8, per = ng + (W % 8 ? 1 : 0);
    if (u >= H * per) return;
    const int y = u / per, g = u - y * per;
    const uint8_t *up = s + (size_t)(2 * y) * W0 * 3, *lo = up + (size_t)W0 * 3;
    uint8_t *o = d + (size_t)y * W * 3;
    if (g < ng) {
      uint32_t a[12], b[12], r[6] = {0, 0, 0, 0, 0, 0};
      io_load(up + g * 48, a);
      io_load(lo + g * 48, b);
#pragma unroll
      for (int j = 0; j < 24; j++) {
        const int k = 6 * (j / 3) + j % 3;     // byte of channel j % 3 of the left source pixel of output pixel j / 3
        r[j >> 2] |= io_box_u8(io_byte(a, k), io_byte(a, k + 3), io_byte(b, k), io_byte(b, k + 3)) << ((j & 3) * 8);
      }
      io_store(o + g * 24, r);
    } else {
      for (int x = ng * 8; x < W; x++)
        for (int c = 0; c < 3; c++)
          o[x * 3 + c] = (uint8_t)io_box_u8(up[6 * x + c], up[6 * x + 3 + c], lo[6 * x + c], lo[6 * x + 3 + c]);
    }
    return;
  }
  if (!src_msk) return;
  const uint8_t *s = src_msk + (size_t)f * src_px;
  float *d = masks + ((size_t)first + f) * dst_px;
  if (factor == 1) {
    const int np = H0 * W0, ng = np / 16;
    if (u < ng) {
      uint32_t w[4];
      float v[16];
      io_load(s + (size_t)u * 16, w);
#pragma unroll
      for (int j = 0; j < 16; j++) v[j] = io_mask1(io_byte(w, j), form);
      io_store_f(d + (size_t)u * 16, v);
    } else if (u == ng) {
      for (int k = ng * 16; k < np; k++) d[k] = io_mask1(s[k], form);
    }
    return;
  }
  const int ng = W / 8, per = ng + (W % 8 ? 1 : 0);
  if (u >= H * per) return;
  const int y = u / per, g = u - y * per;
  const uint8_t *up = s + (size_t)(2 * y) * W0, *lo = up + W0;
  float *o = d + (size_t)y * W;
  if (g < ng) {
    uint32_t a[4], b[4];
    float v[8];
    io_load(up + g * 16, a);
    io_load(lo + g * 16, b);
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = io_mask4(io_byte(a, 2 * j), io_byte(a, 2 * j + 1), io_byte(b, 2 * j), io_byte(b, 2 * j + 1), form);
    io_store_f(o + g * 8, v);
  } else {
    for (int x = ng * 8; x < W; x++) o[x] = io_mask4(up[2 * x], up[2 * x + 1], lo[2 * x], lo[2 * x + 1], form);
  }
}

}  // namespace

extern "C" int ia_io_ingest_chunk(const uint8_t *src_images, const uint8_t *src_masks, int mask_form, int n, int H0, int W0,
                                  int factor, uint8_t *images, float *masks, long long first, long long n_frames, void *stream) {
  IA_CHECK_ARG(n >= 0, "ia_io_ingest_chunk: n < 0");
  if (n == 0) return IA_OK;
  IA_CHECK_ARG(stream != nullptr, "ia_io_ingest_chunk: the ingest runs on a side stream, not on the default stream (stream = NULL)");
  IA_CHECK_ARG(factor == 1 || factor == 2, "ia_io_ingest_chunk: downscale factor %d: only 1 (a copy) and 2 (the 2 x 2 box OpenCV dispatches "
               "INTER_LINEAR to) are restated", factor);
  IA_CHECK_ARG(H0 > 0 && W0 > 0 && (size_t)H0 * W0 * 3 <= (size_t)INT_MAX, "ia_io_ingest_chunk: bad source size %d x %d", H0, W0);
  IA_CHECK_ARG(factor == 1 || (H0 % 2 == 0 && W0 % 2 == 0), "ia_io_ingest_chunk: factor 2 needs an even source size (got %d x %d): "
               "OpenCV's handling of the odd edge is not restated", H0, W0);
  IA_CHECK_ARG(src_images || src_masks, "ia_io_ingest_chunk: neither images nor masks given");
  IA_CHECK_ARG((!src_images || images) && (!src_masks || masks), "ia_io_ingest_chunk: a source without its store");
  IA_CHECK_ARG(!src_masks || mask_form == IA_IO_MASK_U8 || mask_form == IA_IO_MASK_GREY, "ia_io_ingest_chunk: unknown mask form %d", mask_form);
  IA_CHECK_ARG(n <= 65535 && first >= 0 && first + n <= n_frames, "ia_io_ingest_chunk: frames [%lld, %lld) outside the store of %lld frames "
               "(or more than 65535 in a chunk)", first, first + n, n_frames);
  const int H = H0 / factor, W = W0 / factor;
  long units;
  if (factor == 1) units = (long)H0 * W0 * (src_images ? 3 : 1) / 16 + 1;
  else units = (long)H * (W / 8 + (W % 8 ? 1 : 0));
  hipLaunchKernelGGL(k_io_ingest, dim3(ia_div_up(units, 256), 2, n), dim3(256), 0, (hipStream_t)stream, src_images, src_masks, mask_form,
                     H0, W0, factor, images, masks, first);
  IA_LAUNCH_CHECK("k_io_ingest");
  return IA_OK;
}
