// ia_masks.hip -- cleaning raw per-frame segmentation masks (include/instantavatar_hip_masks.h; definition in DESIGN.md section 4,
// "mask cleaning"): threshold, k x k box open and close, connected components, keep the largest.  What the reference does per frame
// with three cv2 passes and a labelling pass (scripts/custom/extract-largest-connected-components.py) is here a fixed number of
// launches for the whole batch: grid.y = frame, grid.x = the 64-pixel words of a frame.
//
// Representation.  A row is bit-packed into Ww = ceil(W / 64) 64-bit words (bit b of word w = pixel x = 64 w + b; the bits at x >= W of
// the last word are kept 0), one wave ballot per word.  Morphology along x is a shift with a carry from the neighbouring word, along
// y an AND / OR over the rows of the window; both happen in one pass per operation, a thread per output word.  open then close is
// erode(r), dilate(r), dilate(r), erode(r) with r = (k - 1) / 2; the two dilations in the middle are ONE dilation by 2 r: with pixels
// outside the image ignored, dilate(r) o dilate(r) at p is the OR over every image pixel s for which an image pixel q with |q - p| <= r
// and |s - q| <= r (per axis) exists, and since the image is a rectangle such a q exists exactly when |s - p| <= 2 r (take q between
// p and s on each axis).  2 r <= 30 < 64, so the carry still comes from the neighbouring word only.
//
// Components are labelled by RUNS, not pixels (the shape of k_occ_runs / k_occ_union_runs in ia_render.hip).  A run is a maximal
// stretch of set bits of a row (it may span words); its id is q = 64 * (y Ww + w) + b of its first pixel, so ids ascend in row-major
// order, and since two runs cannot start at x and x + 1 its union-find cell is parent[q >> 1]: 2 bytes per pixel instead of 4.  The head
// of every run unions it with the runs of the row above that it touches (the overlap widened by one pixel for 8-connectivity).  A
// link always goes from the larger root to the smaller one, so the root of a component is the run of its first pixel whatever the
// order the links were made in: the label.  Areas are integer atomic adds of run lengths onto the root; the kept component is a
// 64-bit atomicMax of (area << 32) | ~root per frame (largest area, then smallest root), as k_occ_best does.
//
// Loop bounds.  No loop waits for another thread: every one has a bound that follows from the sizes, stated where the loop is.  The
// union-find loops carry the bound as an explicit counter as well (`cap` = the cells of a frame >= its runs), so even a corrupted
// parent array ends them.
#include "ia_common.h"
#include "../../include/instantavatar_hip_masks.h"

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ u64 mk_low(int nbits) { return nbits >= 64 ? ~0ull : ((1ull << nbits) - 1ull); }   // bits [0, nbits), 0 <= nbits

// x of the first pixel of the run that holds the set bit b of word w of `row`.  The loop walks back over words that are all ones:
// at most w <= Ww - 1 steps.
__device__ __forceinline__ int mk_run_head(const u64 *__restrict__ row, int w, int b) {
  u64 z = ~row[w] & mk_low(b);
  if (z) return w * 64 + 64 - __clzll((long long)z);
  for (int v = w - 1; v >= 0; v--) {
    z = ~row[v];
    if (z) return v * 64 + 64 - __clzll((long long)z);     // (bit 63 clear: the run starts at word v + 1)
  }
  return 0;
}

// x of its last pixel.  At most Ww - 1 - w steps; the zero bits behind W end a run at the right border.
__device__ __forceinline__ int mk_run_end(const u64 *__restrict__ row, int w, int b, int Ww) {
  u64 z = ~row[w] & ~mk_low(b + 1);
  if (z) return w * 64 + __ffsll((long long)z) - 2;
  for (int v = w + 1; v < Ww; v++) {
    z = ~row[v];
    if (z) return v * 64 + __ffsll((long long)z) - 2;
  }
  return Ww * 64 - 1;       // (only when W is a multiple of 64)
}

// Root of run q.  parent[] only ever changes from "itself" to a SMALLER id, so the chain descends strictly: at most (runs of the
// frame) <= cap steps.
__device__ __forceinline__ int mk_root(int32_t *parent, int q, int cap) {
  for (int s = 0; s < cap; s++) {
    const int p = __hip_atomic_load(&parent[q >> 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == q) break;
    q = p;
  }
  return q;
}

// Link the components of runs a and b, larger root under smaller.  A failed CAS means that root stopped being a root since it was
// found, by somebody else's successful link; a frame sees fewer than `runs` successful links in all, so this thread fails fewer than
// `runs` <= cap times.  Nothing here waits for a value another thread has yet to write.
__device__ __forceinline__ void mk_union(int32_t *parent, int a, int b, int cap) {
  for (int s = 0; s <= cap; s++) {
    a = mk_root(parent, a, cap);
    b = mk_root(parent, b, cap);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    if (atomicCAS(&parent[a >> 1], a, b) == a) return;
  }
}

// ---- 1: threshold + pack.  A wave per word, a lane per pixel ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mask_pack(const uint8_t *__restrict__ src, int H, int W, int Ww, int threshold,
                                                   u64 *__restrict__ bits) {
  const int f = blockIdx.y;
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;     // word of the frame (wave-uniform)
  if (idx >= H * Ww) return;
  const int y = idx / Ww, w = idx - y * Ww, x = w * 64 + lane;
  const bool on = x < W && (int)src[((size_t)f * H + y) * W + x] > threshold;
  const u64 m = __ballot(on);
  if (lane == 0) bits[(size_t)f * H * Ww + idx] = m;
}

// ---- 2: one box erosion (ERODE) or dilation by radius R >= 1, x and y in one pass.  A thread per output word ----------------------
// Loops: 2 R + 1 <= 61 rows, R <= 30 shifts.
template <bool ERODE> __global__ __launch_bounds__(256) void k_mask_morph(const u64 *__restrict__ in, int H, int W, int Ww, int R,
                                                                          u64 *__restrict__ out) {
  const int f = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= H * Ww) return;
  const int y = idx / Ww, w = idx - y * Ww;
  const u64 *fr = in + (size_t)f * H * Ww;
  const u64 valid_last = mk_low(W - (Ww - 1) * 64);          // the bits of the last word that are pixels
  const u64 fill = ERODE ? ~0ull : 0ull;                     // what a pixel outside the image counts as
  u64 acc = fill;
  const int y0 = y - R < 0 ? 0 : y - R, y1 = y + R > H - 1 ? H - 1 : y + R;      // rows outside the image are ignored
  for (int yy = y0; yy <= y1; yy++) {
    const u64 *row = fr + (size_t)yy * Ww;
    u64 c = row[w], p = w > 0 ? row[w - 1] : fill, nx = w < Ww - 1 ? row[w + 1] : fill;
    if (ERODE) {
      if (w == Ww - 1) c |= ~valid_last;
      if (w + 1 == Ww - 1) nx |= ~valid_last;
    }
    u64 a = c;
    for (int d = 1; d <= R; d++) {
      const u64 right = (c >> d) | (nx << (64 - d)), left = (c << d) | (p >> (64 - d));      // pixels x + d and x - d
      a = ERODE ? (a & right & left) : (a | right | left);
    }
    acc = ERODE ? (acc & a) : (acc | a);
  }
  if (w == Ww - 1) acc &= valid_last;
  out[(size_t)f * H * Ww + idx] = acc;
}

// ---- 3: a cell per run head.  A wave per word, a lane per bit (launches 3 to 7) ----------------------------------------------------
struct MaskFrameWs { u64 best; int32_t n_comp; int32_t pad; };

__global__ __launch_bounds__(256) void k_mask_runs(const u64 *__restrict__ bits, int H, int Ww, int32_t *__restrict__ parent,
                                                   int32_t *__restrict__ area, MaskFrameWs *__restrict__ fws) {
  const int f = blockIdx.y;
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (idx >= H * Ww) return;
  const size_t words = (size_t)H * Ww;
  const u64 *fr = bits + f * words;
  if (idx == 0 && lane == 0) { fws[f].best = 0ull; fws[f].n_comp = 0; }
  const u64 m = fr[idx];
  const int w = idx % Ww;
  const bool before = lane > 0 ? (m >> (lane - 1)) & 1ull : (w > 0 ? fr[idx - 1] >> 63 : 0ull);
  if (((m >> lane) & 1ull) && !before) {
    const int q = idx * 64 + lane;
    parent[f * words * 32 + (q >> 1)] = q;
    area[f * words * 32 + (q >> 1)] = 0;
  }
}

// ---- 4: the head of every run unions it with the runs of the row above that it touches ---------------------------------------------
// Loops: the window spans at most Ww words of the row above, a word holds at most 32 runs, and each turn of the inner loop clears at
// least the bit it found.
__global__ __launch_bounds__(256) void k_mask_union(const u64 *__restrict__ bits, int H, int W, int Ww, int widen,
                                                    int32_t *__restrict__ parent) {
  const int f = blockIdx.y;
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (idx >= H * Ww || idx < Ww) return;           // (the first row has nothing above it)
  const size_t words = (size_t)H * Ww;
  const u64 *fr = bits + f * words;
  int32_t *par = parent + f * words * 32;
  const int cap = H * Ww * 32;
  const u64 m = fr[idx];
  const int y = idx / Ww, w = idx - y * Ww;
  const bool before = lane > 0 ? (m >> (lane - 1)) & 1ull : (w > 0 ? fr[idx - 1] >> 63 : 0ull);
  if (!((m >> lane) & 1ull) || before) return;
  const int q = idx * 64 + lane;
  const int x0 = w * 64 + lane, x1 = mk_run_end(fr + (size_t)y * Ww, w, lane, Ww);
  const int lo = x0 - widen < 0 ? 0 : x0 - widen, hi = x1 + widen > W - 1 ? W - 1 : x1 + widen;
  const u64 *up = fr + (size_t)(y - 1) * Ww;
  const int base = (y - 1) * Ww * 64;
  for (int v = lo >> 6; v <= hi >> 6; v++) {
    const u64 um = up[v];
    u64 t = um;
    if (v == lo >> 6) t &= ~mk_low(lo & 63);
    else if (up[v - 1] >> 63) t &= ~mk_low(__ffsll((long long)~um) - 1 < 0 ? 64 : __ffsll((long long)~um) - 1);   // a run met in word v - 1 goes on
    if (v == hi >> 6) t &= mk_low((hi & 63) + 1);
    while (t) {
      const int b = __ffsll((long long)t) - 1;
      const int head = mk_run_head(up, v, b);
      const u64 z = ~um & ~mk_low(b + 1);             // the rest of that run within this word is skipped
      t = z ? t & ~mk_low(__ffsll((long long)z) - 1) : 0ull;
      mk_union(par, q, base + head, cap);
    }
  }
}

// ---- 5: run lengths onto the roots; every run then points straight at its root -----------------------------------------------------
__global__ __launch_bounds__(256) void k_mask_area(const u64 *__restrict__ bits, int H, int Ww, int32_t *__restrict__ parent,
                                                   int32_t *__restrict__ area) {
  const int f = blockIdx.y;
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (idx >= H * Ww) return;
  const size_t words = (size_t)H * Ww;
  const u64 *fr = bits + f * words;
  int32_t *par = parent + f * words * 32;
  const u64 m = fr[idx];
  const int y = idx / Ww, w = idx - y * Ww;
  const bool before = lane > 0 ? (m >> (lane - 1)) & 1ull : (w > 0 ? fr[idx - 1] >> 63 : 0ull);
  if (!((m >> lane) & 1ull) || before) return;
  const int q = idx * 64 + lane;
  const int len = mk_run_end(fr + (size_t)y * Ww, w, lane, Ww) - (w * 64 + lane) + 1;
  const int root = mk_root(par, q, H * Ww * 32);
  atomicAdd(&area[f * words * 32 + (root >> 1)], len);
  // the unions are complete, so `root` is final: a concurrent mk_root reads the old ancestor or the root, both on its way
  if (root != q) __hip_atomic_store(&par[q >> 1], root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- 6: the roots of a frame vote ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mask_best(const u64 *__restrict__ bits, int H, int Ww, const int32_t *__restrict__ parent,
                                                   const int32_t *__restrict__ area, MaskFrameWs *__restrict__ fws) {
  const int f = blockIdx.y;
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (idx >= H * Ww) return;
  const size_t words = (size_t)H * Ww;
  const u64 *fr = bits + f * words;
  const u64 m = fr[idx];
  const int w = idx % Ww;
  const bool before = lane > 0 ? (m >> (lane - 1)) & 1ull : (w > 0 ? fr[idx - 1] >> 63 : 0ull);
  const int q = idx * 64 + lane;
  const bool root = ((m >> lane) & 1ull) && !before && parent[f * words * 32 + (q >> 1)] == q;
  if (root) atomicMax(&fws[f].best, ((u64)(uint32_t)area[f * words * 32 + (q >> 1)] << 32) | (u64)(0xffffffffu - (uint32_t)q));
  const u64 roots = __ballot(root);
  if (roots && lane == 0) atomicAdd(&fws[f].n_comp, __popcll(roots));
}

// ---- 7: the outputs.  A lane per pixel ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mask_write(const u64 *__restrict__ bits, int H, int W, int Ww, int32_t *__restrict__ parent,
                                                    const MaskFrameWs *__restrict__ fws, uint8_t *__restrict__ masks,
                                                    uint8_t *__restrict__ binary, int32_t *__restrict__ labels,
                                                    int32_t *__restrict__ area_out, int32_t *__restrict__ n_components) {
  const int f = blockIdx.y;
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (idx >= H * Ww) return;
  const size_t words = (size_t)H * Ww;
  const u64 *fr = bits + f * words;
  const u64 best = fws[f].best;
  if (idx == 0 && lane == 0) { area_out[f] = (int32_t)(best >> 32); n_components[f] = fws[f].n_comp; }
  const int y = idx / Ww, w = idx - y * Ww, x = w * 64 + lane;
  if (x >= W) return;
  const int winner = best ? (int)(0xffffffffu - (uint32_t)(best & 0xffffffffull)) : -1;
  const bool on = (fr[idx] >> lane) & 1ull;
  int root = -1;
  if (on) root = mk_root(parent + f * words * 32, (y * Ww) * 64 + mk_run_head(fr + (size_t)y * Ww, w, lane), H * Ww * 32);
  const size_t p = ((size_t)f * H + y) * W + x;
  masks[p] = on && root == winner ? 255 : 0;
  if (binary) binary[p] = on ? 255 : 0;
  if (labels) {
    const int ry = (root >> 6) / Ww;
    labels[p] = on ? 1 + ry * W + (root - ry * Ww * 64) : 0;
  }
}

// ---- ia_mask_apply: a thread per 4 pixels (12 image bytes) ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mask_apply(const uint8_t *images, const uint8_t *__restrict__ masks, size_t n_px, int wide,
                                                    uint8_t *out) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, p0 = g * 4;
  if (p0 >= n_px) return;
  if (wide && p0 + 4 <= n_px) {
    const uint32_t mk = ((const uint32_t *)masks)[g];
    const uint32_t *s = (const uint32_t *)images + g * 3;
    uint32_t a = s[0], b = s[1], c = s[2];
    // bytes 0..11 = pixels 0 0 0 1 | 1 1 2 2 | 2 3 3 3
    const uint32_t k0 = mk & 0xffu ? 0xffffffffu : 0u, k1 = mk & 0xff00u ? 0xffffffffu : 0u, k2 = mk & 0xff0000u ? 0xffffffffu : 0u,
                   k3 = mk & 0xff000000u ? 0xffffffffu : 0u;
    a &= (k0 & 0x00ffffffu) | (k1 & 0xff000000u);
    b &= (k1 & 0x0000ffffu) | (k2 & 0xffff0000u);
    c &= (k2 & 0x000000ffu) | (k3 & 0xffffff00u);
    uint32_t *d = (uint32_t *)out + g * 3;
    d[0] = a; d[1] = b; d[2] = c;
    return;
  }
  for (size_t p = p0; p < n_px && p < p0 + 4; p++) {
    const bool keep = masks[p] != 0;
    const uint8_t r = images[p * 3], gg = images[p * 3 + 1], bb = images[p * 3 + 2];
    out[p * 3] = keep ? r : 0; out[p * 3 + 1] = keep ? gg : 0; out[p * 3 + 2] = keep ? bb : 0;
  }
}

struct MaskLayout { size_t bits_a, bits_b, parent, area, frames, total; };

// the one place the workspace is laid out: sizes and offsets, 256-byte aligned pieces
bool mask_layout(int n, int H, int W, MaskLayout *L) {
  if (n < 1 || n > IA_MASK_MAX_FRAMES || H < 1 || W < 1) return false;
  const long long Ww = ((long long)W + 63) / 64;
  if ((long long)H * Ww * 64 >= (1ll << 31)) return false;
  const size_t words = (size_t)n * H * Ww;
  size_t off = 0;
  L->bits_a = off; off += ia_align(words * 8);
  L->bits_b = off; off += ia_align(words * 8);
  L->parent = off; off += ia_align(words * 32 * 4);
  L->area = off; off += ia_align(words * 32 * 4);
  L->frames = off; off += ia_align((size_t)n * sizeof(MaskFrameWs));
  L->total = off;
  return true;
}

bool overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && x < y + nb && y < x + na;
}

}  // namespace

extern "C" size_t ia_mask_clean_workspace_bytes(int n, int H, int W) {
  MaskLayout L;
  return mask_layout(n, H, W, &L) ? L.total : 0;
}

extern "C" int ia_mask_clean(const uint8_t *src, int n, int H, int W, int threshold, int kernel_size, int connectivity, uint8_t *masks,
                             uint8_t *binary, int32_t *labels, int32_t *area, int32_t *n_components, void *ws, size_t ws_bytes,
                             void *stream) {
  IA_CHECK_ARG(n >= 0, "ia_mask_clean: n < 0");
  if (n == 0) return IA_OK;
  IA_CHECK_ARG(stream != nullptr, "ia_mask_clean: an explicit stream is required (stream = NULL)");
  MaskLayout L;
  IA_CHECK_ARG(mask_layout(n, H, W, &L), "ia_mask_clean: %d frames of %d x %d: outside 1 <= n <= %d, H, W >= 1, H * round_up(W, 64) < 2^31",
               n, H, W, IA_MASK_MAX_FRAMES);
  IA_CHECK_ARG(kernel_size >= 1 && kernel_size <= IA_MASK_MAX_KERNEL && (kernel_size & 1),
               "ia_mask_clean: kernel_size %d: the box is odd and in [1, %d]", kernel_size, IA_MASK_MAX_KERNEL);
  IA_CHECK_ARG(connectivity == 8 || connectivity == 4, "ia_mask_clean: connectivity %d: 8 or 4", connectivity);
  IA_CHECK_ARG(threshold >= 0 && threshold <= 255, "ia_mask_clean: threshold %d outside [0, 255] (foreground is src > threshold)", threshold);
  IA_CHECK_ARG(src && masks && area && n_components, "ia_mask_clean: src, masks, area and n_components are required");
  IA_CHECK_ARG(ws && ws_bytes >= L.total, "ia_mask_clean: workspace of %zu bytes, %zu needed (ia_mask_clean_workspace_bytes)",
               ws ? ws_bytes : (size_t)0, L.total);
  IA_CHECK_ARG(((uintptr_t)ws & 7) == 0 && (!labels || ((uintptr_t)labels & 3) == 0) && ((uintptr_t)area & 3) == 0 &&
               ((uintptr_t)n_components & 3) == 0, "ia_mask_clean: ws must be 8-byte aligned, labels / area / n_components 4-byte aligned");
  const size_t px = (size_t)n * H * W;
  IA_CHECK_ARG(!overlap(src, px, masks, px) && !overlap(src, px, binary, px) && !overlap(src, px, labels, px * 4) &&
               !overlap(masks, px, binary, px), "ia_mask_clean: an output overlaps src, or binary overlaps masks");
  const hipStream_t s = (hipStream_t)stream;
  const int Ww = (W + 63) / 64, words = H * Ww;
  char *b = (char *)ws;
  u64 *A = (u64 *)(b + L.bits_a), *B = (u64 *)(b + L.bits_b);
  int32_t *parent = (int32_t *)(b + L.parent), *ar = (int32_t *)(b + L.area);
  MaskFrameWs *fws = (MaskFrameWs *)(b + L.frames);
  const dim3 blk(256), gw(ia_div_up(words, 4), n), gt(ia_div_up(words, 256), n);      // a wave / a thread per word; grid.y = frame
  hipLaunchKernelGGL(k_mask_pack, gw, blk, 0, s, src, H, W, Ww, threshold, A);
  IA_LAUNCH_CHECK("k_mask_pack");
  const int r = (kernel_size - 1) / 2;
  if (r > 0) {
    hipLaunchKernelGGL(k_mask_morph<true>, gt, blk, 0, s, (const u64 *)A, H, W, Ww, r, B);
    hipLaunchKernelGGL(k_mask_morph<false>, gt, blk, 0, s, (const u64 *)B, H, W, Ww, 2 * r, A);
    hipLaunchKernelGGL(k_mask_morph<true>, gt, blk, 0, s, (const u64 *)A, H, W, Ww, r, B);
    IA_LAUNCH_CHECK("k_mask_morph");
  }
  const u64 *bits = r > 0 ? B : A;
  hipLaunchKernelGGL(k_mask_runs, gw, blk, 0, s, bits, H, Ww, parent, ar, fws);
  hipLaunchKernelGGL(k_mask_union, gw, blk, 0, s, bits, H, W, Ww, connectivity == 8 ? 1 : 0, parent);
  hipLaunchKernelGGL(k_mask_area, gw, blk, 0, s, bits, H, Ww, parent, ar);
  hipLaunchKernelGGL(k_mask_best, gw, blk, 0, s, bits, H, Ww, (const int32_t *)parent, (const int32_t *)ar, fws);
  hipLaunchKernelGGL(k_mask_write, gw, blk, 0, s, bits, H, W, Ww, parent, (const MaskFrameWs *)fws, masks, binary, labels, area,
                     n_components);
  IA_LAUNCH_CHECK("k_mask_write");
  return IA_OK;
}

extern "C" int ia_mask_apply(const uint8_t *images, const uint8_t *masks, int n, int H, int W, uint8_t *out, void *stream) {
  IA_CHECK_ARG(n >= 0, "ia_mask_apply: n < 0");
  if (n == 0) return IA_OK;
  IA_CHECK_ARG(stream != nullptr, "ia_mask_apply: an explicit stream is required (stream = NULL)");
  IA_CHECK_ARG(H >= 1 && W >= 1 && n <= IA_MASK_MAX_FRAMES, "ia_mask_apply: %d frames of %d x %d", n, H, W);
  IA_CHECK_ARG(images && masks && out, "ia_mask_apply: images, masks and out are required");
  const size_t px = (size_t)n * H * W;
  IA_CHECK_ARG(px / 4 / 256 < (size_t)INT_MAX, "ia_mask_apply: %zu pixels are too many for one launch", px);
  IA_CHECK_ARG(out == images || !overlap(images, px * 3, out, px * 3), "ia_mask_apply: out may be images itself, not overlap it otherwise");
  IA_CHECK_ARG(!overlap(masks, px, out, px * 3), "ia_mask_apply: out overlaps masks");
  const int wide = (((uintptr_t)images | (uintptr_t)masks | (uintptr_t)out) & 3) == 0;
  hipLaunchKernelGGL(k_mask_apply, dim3(ia_div_up((long)((px + 3) / 4), 256)), dim3(256), 0, (hipStream_t)stream, images, masks, px, wide, out);
  IA_LAUNCH_CHECK("k_mask_apply");
  return IA_OK;
}
