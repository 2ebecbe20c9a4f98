// ia_png.hip -- PNG filtering and deflate of a batch of 8-bit frames (include/instantavatar_hip_png.h; definition in DESIGN.md section 4,
// "PNG encoding").  What the drivers did per frame with PIL on host threads is here two stages for the whole batch:
//   k_png_strip    grid (strip, image), one workgroup of 16 waves per strip.  The strip's filtered bytes live in LDS; the workgroup
//                  filters (a wave per row), finds the runs, counts the symbols, builds the codes, and writes the strip's piece of the
//                  deflate stream into the strip's own slot of the workspace
//   ia_scan + k_png_gather   the exclusive scan of the pieces' sizes (ia_scan.h), then grid (strip, image) again: every piece is copied to
//                  its place in `out`; the first strip of an image also writes 78 01 and the image's offset, the last one the Adler-32
//
// Tokens are never stored.  Thread t owns the bytes [t Q, (t + 1) Q) of the strip, Q = ceil(L / 1024).  Which tokens START in its chunk
// follows from the chunk's bytes and two numbers: the last run head before the chunk (a max-scan over the threads) and the first one
// behind it (a min-scan from the other end) -- the segmented scan of the definition.  The thread then walks its chunk three times with
// the same routine (png_walk): to count symbols, to add up code lengths (prefix sum -> its bit offset), to write its codes.  Bits are
// written with atomicOr on 32-bit words of the slot, zeroed by the workgroup before: OR is commutative, the bytes do not depend on
// the order.  The same holds for the integer atomicAdds of the histogram and of the Adler sums.
//
// Serial parts (one lane, the others wait at a barrier): Huffman's merge over at most 286 sorted leaves, the length limit, the
// code-length tokens (at most 288) and their 19-symbol code.  What is a fixed 286 trips long is done by a lane per symbol instead: the
// sort (a rank count), the number of used symbols and HLIT, the canonical literal/length codes and the block's size in bits.
//
// Loop bounds.  No loop waits for another thread.  Every loop runs over a range fixed by the sizes (bytes of a chunk, symbols of an
// alphabet, strips of an image); the limit loop ends because the Kraft sum drops by one per trip and starts below 2^16.
#include "ia_common.h"
#include "ia_scan.h"
#include "../../include/instantavatar_hip_png.h"

namespace {

typedef unsigned long long u64;

#define PNG_THREADS 1024
#define PNG_WAVES (PNG_THREADS / 64)
#define PNG_ADLER 65521u
#define PNG_STORED_MAX 65535
#define PNG_NLIT 286
#define PNG_NCL 19
#define PNG_MAX_CLTOK 296      // code-length tokens: at most one per length of the sequence (286 + 2), rounded up

__device__ __forceinline__ int png_stored_bytes(int L) { return L + 5 * ((L + PNG_STORED_MAX - 1) / PNG_STORED_MAX); }
static inline long long png_stored_bytes_host(long long L) { return L + 5 * ((L + PNG_STORED_MAX - 1) / PNG_STORED_MAX); }

// match length 3 .. 258 -> its symbol, the number of extra bits and their value (RFC 1951 3.2.5, computed: from x = len - 3 >= 8 on
// the codes come in groups of four per power of two)
__device__ __forceinline__ void png_length_code(int len, int &sym, int &eb, int &ev) {
  const int x = len - 3;
  if (x < 8) { sym = 257 + x; eb = 0; ev = 0; return; }
  if (x == 255) { sym = 285; eb = 0; ev = 0; return; }
  eb = 29 - __clz(x);                       // floor(log2 x) - 2
  sym = 261 + 4 * eb + ((x >> eb) & 3);
  ev = x & ((1 << eb) - 1);
}

// ---- the workgroup's scans over one int per thread ---------------------------------------------------------------------------------------
// exclusive running maximum (of values >= -1; -1 in front of thread 0).  s_w: PNG_WAVES ints nobody still reads; barrier inside
__device__ __forceinline__ int png_excl_max(int v, int *s_w) {
  const int lane = ia_lane(), wave = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x = x > y ? x : y;
  }
  if (lane == 63) s_w[wave] = x;
  int ex = __shfl_up(x, 1, 64);
  if (lane == 0) ex = -1;
  __syncthreads();
  for (int w = 0; w < wave; w++) ex = ex > s_w[w] ? ex : s_w[w];
  __syncthreads();
  return ex;
}
// exclusive running minimum from the other end (`top` behind the last thread)
__device__ __forceinline__ int png_excl_min_rev(int v, int top, int *s_w) {
  const int lane = ia_lane(), wave = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_down(x, o, 64);
    if (lane + o < 64) x = x < y ? x : y;
  }
  if (lane == 0) s_w[wave] = x;
  int ex = __shfl_down(x, 1, 64);
  if (lane == 63) ex = top;
  __syncthreads();
  for (int w = wave + 1; w < PNG_WAVES; w++) ex = ex < s_w[w] ? ex : s_w[w];
  __syncthreads();
  return ex;
}
// exclusive prefix sum and the total
__device__ __forceinline__ int png_excl_sum(int v, int *s_w, int &total) {
  const int wave = threadIdx.x >> 6;
  int wave_total;
  const int x = ia_wave_excl_scan(v, wave_total);
  if (ia_lane() == 0) s_w[wave] = wave_total;
  __syncthreads();
  int base = 0;
  total = 0;
  for (int w = 0; w < PNG_WAVES; w++) {
    if (w < wave) base += s_w[w];
    total += s_w[w];
  }
  __syncthreads();
  return base + x;
}

// ---- tokens ------------------------------------------------------------------------------------------------------------------------------
// Calls f.lit(byte) / f.match(length) for every token that STARTS in [c0, c1), in order.  prev_head: the last run head before c0 (used
// when c0 is no head itself), next_head: the first run head at or behind c1 (L when there is none).
// Loops: the bytes of the chunk once; the matches of 258 that start in it (at most 1 + (c1 - c0) / 258).
template <class F> __device__ __forceinline__ void png_walk(const uint8_t *s, int c0, int c1, int prev_head, int next_head, F &f) {
  int i = c0;
  if (i >= c1) return;
  int p = (i == 0 || s[i] != s[i - 1]) ? i : prev_head;        // head of the run that holds i
  while (i < c1) {
    int j = i + 1;
    while (j < c1 && s[j] == s[j - 1]) j++;
    const int e = j < c1 ? j : next_head;                      // the run is [p, e)
    const int lim = e < c1 ? e : c1;
    const int v = s[i];
    if (p == i) f.lit(v);
    const int m = e - p - 1, q = m / 258, r = m - q * 258;
    const int t0 = p + 1, lo = i > t0 ? i : t0;                 // the run's tail starts at t0; ours at lo
    for (int a = (lo - t0 + 257) / 258; a < q && t0 + 258 * a < lim; a++) f.match(258);
    const int R = t0 + 258 * q;                                // where the remainder starts
    if (r >= 3) {
      if (R >= lo && R < lim) f.match(r);
    } else {
      for (int x = R > lo ? R : lo; x < lim && x < R + r; x++) f.lit(v);
    }
    i = lim;
    p = i;
  }
}

struct PngCount {                 // symbols into the histogram
  unsigned *hist;
  __device__ __forceinline__ void lit(int v) { atomicAdd(&hist[v], 1u); }
  __device__ __forceinline__ void match(int len) {
    int sym, eb, ev;
    png_length_code(len, sym, eb, ev);
    atomicAdd(&hist[sym], 1u);
  }
};
struct PngBits {                  // code lengths added up
  const unsigned *code;           // reversed code | length << 16
  int bits;
  __device__ __forceinline__ void lit(int v) { bits += code[v] >> 16; }
  __device__ __forceinline__ void match(int len) {
    int sym, eb, ev;
    png_length_code(len, sym, eb, ev);
    bits += (code[sym] >> 16) + eb + 1;
  }
};
// LSB-first bit output into zeroed words.  A put is at most 32 bits.
struct PngOut {
  unsigned *w;
  int words;                      // of the slot: nothing is written behind them
  int idx, n;
  u64 acc;
  __device__ __forceinline__ void begin(unsigned *words_, int cap, long long bitpos) {
    w = words_; words = cap; idx = (int)(bitpos >> 5); n = (int)(bitpos & 31); acc = 0;
  }
  __device__ __forceinline__ void flush() {
    while (n >= 32) {
      if ((unsigned)acc != 0u && idx < words) atomicOr(&w[idx], (unsigned)acc);
      acc >>= 32; n -= 32; idx++;
    }
  }
  __device__ __forceinline__ void put(unsigned v, int bits) { acc |= (u64)v << n; n += bits; flush(); }
  __device__ __forceinline__ void align() { n = (n + 7) & ~7; flush(); }
  __device__ __forceinline__ void end() {
    if (n > 0 && (unsigned)acc != 0u && idx < words) atomicOr(&w[idx], (unsigned)acc);
  }
};
struct PngEmit {
  const unsigned *code;
  PngOut out;
  __device__ __forceinline__ void lit(int v) { const unsigned c = code[v]; out.put(c & 0xffffu, (int)(c >> 16)); }
  __device__ __forceinline__ void match(int len) {
    int sym, eb, ev;
    png_length_code(len, sym, eb, ev);
    const unsigned c = code[sym];
    const int cl = (int)(c >> 16);
    out.put((c & 0xffffu) | ((unsigned)ev << cl), cl + eb + 1);       // code, extra bits, the distance code 0 (one zero bit)
  }
};

// ---- code construction (one lane) ----------------------------------------------------------------------------------------------------------
struct PngTreeWs {                // scratch of png_build_lengths
  unsigned iw[PNG_NLIT];
  uint16_t leaf_parent[PNG_NLIT], int_parent[PNG_NLIT];
  uint8_t idepth[PNG_NLIT];
  int c[17], next[17];            // leaves per depth; codes per length
};
// order[0 .. u): the used symbols ascending by (frequency, symbol), u >= 2 -> lens[] of them (the others are left as they are).
// Loops: u - 1 merges, u depths, the limit loop (see the head of the file), u lengths.
__device__ void png_build_lengths(const unsigned *freq, const uint16_t *order, int u, int limit, uint8_t *lens, PngTreeWs &T) {
  int li = 0, ii = 0;
  for (int ni = 0; ni < u - 1; ni++) {
    unsigned tot = 0;
    for (int k = 0; k < 2; k++) {
      if (li < u && (ii >= ni || freq[order[li]] <= T.iw[ii])) { tot += freq[order[li]]; T.leaf_parent[li++] = (uint16_t)ni; }
      else { tot += T.iw[ii]; T.int_parent[ii++] = (uint16_t)ni; }
    }
    T.iw[ni] = tot;
  }
  T.idepth[u - 2] = 0;
  for (int k = u - 3; k >= 0; k--) T.idepth[k] = (uint8_t)(T.idepth[T.int_parent[k]] + 1);      // (a parent is made after its children)
  int *c = T.c;
  for (int d = 0; d <= 16; d++) c[d] = 0;
  for (int k = 0; k < u; k++) {
    const int d = T.idepth[T.leaf_parent[k]] + 1;
    c[d < limit ? d : limit]++;
  }
  int total = 0;
  for (int d = 1; d <= limit; d++) total += c[d] << (limit - d);
  while (total > (1 << limit)) {
    c[limit]--;
    for (int d = limit - 1; d > 0; d--)
      if (c[d]) { c[d]--; c[d + 1] += 2; break; }
    total--;
  }
  int j = u;
  for (int d = 1; d <= limit; d++)
    for (int k = 0; k < c[d] && j > 0; k++) lens[order[--j]] = (uint8_t)d;
}
// canonical codes, bit-reversed for the LSB-first stream, packed with their lengths
__device__ void png_make_codes(const uint8_t *lens, int n, int limit, unsigned *code, PngTreeWs &T) {
  int *bl = T.c, *next = T.next;
  for (int b = 0; b <= 16; b++) bl[b] = 0;
  for (int s = 0; s < n; s++) bl[lens[s]]++;
  bl[0] = 0;
  int c = 0;
  next[0] = 0;
  for (int b = 1; b <= limit; b++) { c = (c + bl[b - 1]) << 1; next[b] = c; }
  for (int s = 0; s < n; s++) {
    const int l = lens[s];
    code[s] = l ? ((__brev((unsigned)next[l]++) >> (32 - l)) | ((unsigned)l << 16)) : 0u;
  }
}

__constant__ uint8_t c_cl_order[PNG_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct PngShared {
  unsigned hist[PNG_NLIT + 2];
  unsigned code[PNG_NLIT + 2];
  uint16_t order[PNG_NLIT + 2];
  uint8_t lens[PNG_NLIT + 2];         // literal/length code lengths, then the two distance lengths
  PngTreeWs tree;
  uint8_t cl_sym[PNG_MAX_CLTOK], cl_ext[PNG_MAX_CLTOK];
  unsigned cl_freq[PNG_NCL], cl_code[PNG_NCL];
  uint16_t cl_order[PNG_NCL];
  uint8_t cl_lens[PNG_NCL];
  int scan[PNG_WAVES];
  unsigned adler_a, adler_b, body_bits;
  int ll_next[16];
  int n_used, n_cltok, hlit, hclen, hdr_bits, kind, size;
};

// ---- pixels ------------------------------------------------------------------------------------------------------------------------------
template <int C> __device__ __forceinline__ int png_px(const uint8_t *__restrict__ row, int x, bool swap) {
  if (swap) {
    const int c = C == 4 ? (x & 3) : (x % 3);
    x += c == 0 ? 2 : (c == 2 ? -2 : 0);
  }
  return row[x];
}
__device__ __forceinline__ int png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ int png_abs8(int f) { f &= 255; return f < 128 ? f : 256 - f; }

struct PngArgs {
  const uint8_t *images;
  int H, W, strip_rows, swap_rb, S;
  uint8_t *slots; size_t slot_stride;
  int32_t *sizes, *kinds;
  unsigned *adler_a, *adler_b;
};

template <int C> __global__ __launch_bounds__(PNG_THREADS) void k_png_strip(PngArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_bytes[];
  __shared__ PngShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int strip = blockIdx.x, img = blockIdx.y;
  const int r0 = strip * A.strip_rows, rows = min(A.strip_rows, A.H - r0);
  const int B = A.W * C, row = B + 1, L = rows * row;
  const bool last = strip == A.S - 1, swap = A.swap_rb != 0;
  const uint8_t *im = A.images + (size_t)img * A.H * B;
  const size_t sidx = (size_t)img * A.S + strip;
  uint8_t *slot = A.slots + sidx * A.slot_stride;

  // ---- 1: filter, a wave per row.  Loops: rows / 16 rows, B / 64 bytes, twice
  for (int r = wave; r < rows; r += PNG_WAVES) {
    const int y = r0 + r;
    const uint8_t *cur = im + (size_t)y * B, *up = cur - B;       // (up is only read when y > 0)
    int cost[5] = {0, 0, 0, 0, 0};
    for (int x = lane; x < B; x += 64) {
      const int v = png_px<C>(cur, x, swap), a = x >= C ? png_px<C>(cur, x - C, swap) : 0;
      const int b = y > 0 ? png_px<C>(up, x, swap) : 0, c = (y > 0 && x >= C) ? png_px<C>(up, x - C, swap) : 0;
      cost[0] += png_abs8(v); cost[1] += png_abs8(v - a); cost[2] += png_abs8(v - b);
      cost[3] += png_abs8(v - ((a + b) >> 1)); cost[4] += png_abs8(v - png_paeth(a, b, c));
    }
    int best = 0, best_cost = 0;
#pragma unroll
    for (int t = 0; t < 5; t++) {
      int s = cost[t];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (t == 0 || s < best_cost) { best = t; best_cost = s; }
    }
    uint8_t *dst = s_bytes + r * row;
    if (lane == 0) dst[0] = (uint8_t)best;
    for (int x = lane; x < B; x += 64) {
      const int v = png_px<C>(cur, x, swap), a = x >= C ? png_px<C>(cur, x - C, swap) : 0;
      const int b = y > 0 ? png_px<C>(up, x, swap) : 0, c = (y > 0 && x >= C) ? png_px<C>(up, x - C, swap) : 0;
      const int pred = best == 0 ? 0 : best == 1 ? a : best == 2 ? b : best == 3 ? ((a + b) >> 1) : png_paeth(a, b, c);
      dst[1 + x] = (uint8_t)(v - pred);
    }
  }
  for (int s = tid; s < PNG_NLIT + 2; s += PNG_THREADS) { sh.hist[s] = 0; sh.lens[s] = 0; sh.code[s] = 0; }
  if (tid == 0) { sh.adler_a = 0; sh.adler_b = 0; sh.n_used = 0; sh.hlit = 257; sh.body_bits = 0; }
  __syncthreads();

  // ---- 2: the chunk's run heads and its part of the Adler sums
  const int Q = (L + PNG_THREADS - 1) / PNG_THREADS;
  const int c0 = min(L, tid * Q), c1 = min(L, c0 + Q);
  int last_head = -1, first_head = L;
  {
    u64 sa = 0, sb = 0;
    for (int i = c0; i < c1; i++) {
      const unsigned v = s_bytes[i];
      if (i == 0 || v != s_bytes[i - 1]) { last_head = i; if (first_head == L) first_head = i; }
      sa += v; sb += (u64)(L - i) * v;
    }
    if (c1 > c0) { atomicAdd(&sh.adler_a, (unsigned)(sa % PNG_ADLER)); atomicAdd(&sh.adler_b, (unsigned)(sb % PNG_ADLER)); }
  }
  const int prev_head = png_excl_max(last_head, sh.scan);
  const int next_head = png_excl_min_rev(first_head, L, sh.scan);

  // ---- 3: histogram
  {
    PngCount f{sh.hist};
    png_walk(s_bytes, c0, c1, prev_head, next_head, f);
    if (tid == 0) atomicAdd(&sh.hist[256], 1u);
  }
  __syncthreads();

  // ---- 4: codes.  The used symbols are ranked in parallel (286 comparisons each), the rest is one lane's
  if (tid < PNG_NLIT) {
    const unsigned f = sh.hist[tid];
    if (f) {
      int rank = 0;
      for (int t = 0; t < PNG_NLIT; t++) {
        const unsigned g = sh.hist[t];
        rank += (g != 0u && (g < f || (g == f && t < tid))) ? 1 : 0;
      }
      sh.order[rank] = (uint16_t)tid;
      atomicAdd(&sh.n_used, 1);
      if (tid >= 257) atomicMax(&sh.hlit, tid + 1);           // (a used symbol is one with a code length)
    }
  }
  __syncthreads();
  if (tid == 0) {
    png_build_lengths(sh.hist, sh.order, sh.n_used, 15, sh.lens, sh.tree);
    {                                                         // first code of every length (RFC 1951 3.2.2) from the leaves per length
      int c = 0;
      sh.ll_next[0] = 0;
      for (int b = 1; b <= 15; b++) { c = (c + (b > 1 ? sh.tree.c[b - 1] : 0)) << 1; sh.ll_next[b] = c; }
    }
    const int hlit = sh.hlit;
    sh.lens[hlit] = 1; sh.lens[hlit + 1] = 1;                 // the distance alphabet, behind the HLIT lengths
    // code-length tokens over lens[0 .. hlit + 2)
    for (int s = 0; s < PNG_NCL; s++) { sh.cl_freq[s] = 0; sh.cl_lens[s] = 0; }
    const int nseq = hlit + 2;
    int nt = 0;
    for (int i = 0; i < nseq;) {
      const int v = sh.lens[i];
      int j = i;
      while (j < nseq && sh.lens[j] == v) j++;
      int k = j - i;
      if (v == 0) {
        while (k >= 11) { const int c = k < 138 ? k : 138; sh.cl_sym[nt] = 18; sh.cl_ext[nt++] = (uint8_t)(c - 11); k -= c; }
        if (k >= 3) { sh.cl_sym[nt] = 17; sh.cl_ext[nt++] = (uint8_t)(k - 3); k = 0; }
        for (; k > 0; k--) { sh.cl_sym[nt] = 0; sh.cl_ext[nt++] = 0; }
      } else {
        sh.cl_sym[nt] = (uint8_t)v; sh.cl_ext[nt++] = 0; k--;
        while (k >= 3) { const int c = k < 6 ? k : 6; sh.cl_sym[nt] = 16; sh.cl_ext[nt++] = (uint8_t)(c - 3); k -= c; }
        for (; k > 0; k--) { sh.cl_sym[nt] = (uint8_t)v; sh.cl_ext[nt++] = 0; }
      }
      i = j;
    }
    for (int t = 0; t < nt; t++) sh.cl_freq[sh.cl_sym[t]]++;
    int cu = 0;                                               // the used code-length symbols, insertion-sorted by (frequency, symbol)
    for (int s = 0; s < PNG_NCL; s++) {
      if (!sh.cl_freq[s]) continue;
      int k = cu++;
      for (; k > 0 && sh.cl_freq[sh.cl_order[k - 1]] > sh.cl_freq[s]; k--) sh.cl_order[k] = sh.cl_order[k - 1];
      sh.cl_order[k] = (uint16_t)s;
    }
    png_build_lengths(sh.cl_freq, sh.cl_order, cu, 7, sh.cl_lens, sh.tree);
    int hclen = 4;
    for (int k = 4; k < PNG_NCL; k++) if (sh.cl_lens[c_cl_order[k]]) hclen = k + 1;
    sh.lens[hlit] = 0; sh.lens[hlit + 1] = 0;                 // (the table of literal/length codes below has no use for them)
    png_make_codes(sh.cl_lens, PNG_NCL, 7, sh.cl_code, sh.tree);
    long long bits = 17 + 3 * hclen;
    for (int t = 0; t < nt; t++) {
      const int s = sh.cl_sym[t];
      bits += sh.cl_lens[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
    }
    sh.hdr_bits = (int)bits;
    sh.n_cltok = nt; sh.hclen = hclen;
  }
  __syncthreads();
  // the literal/length codes and the bits of all tokens, a lane per symbol: a symbol's canonical code is the first code of its length
  // plus the number of lower symbols of that length (286 comparisons each)
  if (tid < PNG_NLIT) {
    const int l = sh.lens[tid];
    if (l) {
      int before = 0;
      for (int t = 0; t < tid; t++) before += sh.lens[t] == l ? 1 : 0;
      sh.code[tid] = (__brev((unsigned)(sh.ll_next[l] + before)) >> (32 - l)) | ((unsigned)l << 16);
      const int k = tid - 257, eb = k < 8 ? 0 : (k == 28 ? 0 : (k - 4) >> 2);       // matches: extra bits and the distance bit
      atomicAdd(&sh.body_bits, sh.hist[tid] * (unsigned)(l + (tid > 256 ? eb + 1 : 0)));
    }
  }
  __syncthreads();
  if (tid == 0) {
    long long bits = (long long)sh.hdr_bits + sh.body_bits;
    if (!last) bits = ((bits + 3 + 7) & ~7ll) + 32;
    const long long coded = (bits + 7) >> 3;
    const int stored = png_stored_bytes(L);
    sh.kind = coded > stored ? 1 : 0;
    sh.size = sh.kind ? stored : (int)coded;
  }
  __syncthreads();
  const int kind = sh.kind, size = sh.size;
  if (tid == 0) {
    A.sizes[sidx] = size; A.kinds[sidx] = kind;
    A.adler_a[sidx] = sh.adler_a % PNG_ADLER; A.adler_b[sidx] = sh.adler_b % PNG_ADLER;
  }

  if (kind) {
    // ---- 5b: stored blocks.  Byte i of the strip goes behind the headers of the blocks up to its own
    const int nblk = (L + PNG_STORED_MAX - 1) / PNG_STORED_MAX;
    for (int i = tid; i < L; i += PNG_THREADS) slot[i + 5 * (i / PNG_STORED_MAX + 1)] = s_bytes[i];
    if (tid < nblk) {
      const int len = min(PNG_STORED_MAX, L - tid * PNG_STORED_MAX);
      uint8_t *h = slot + (size_t)tid * (PNG_STORED_MAX + 5);
      h[0] = (last && tid == nblk - 1) ? 1 : 0;
      h[1] = (uint8_t)(len & 255); h[2] = (uint8_t)(len >> 8); h[3] = (uint8_t)(~len & 255); h[4] = (uint8_t)((~len >> 8) & 255);
    }
    return;
  }

  // ---- 5a: the dynamic block.  The slot's words are zeroed, every thread finds its bit offset, then ORs its codes in
  unsigned *words = (unsigned *)slot;
  const int nwords = (size + 3) >> 2;                         // <= slot_stride / 4: size <= the stored size
  for (int i = tid; i < nwords; i += PNG_THREADS) words[i] = 0u;
  PngBits fb{sh.code, 0};
  png_walk(s_bytes, c0, c1, prev_head, next_head, fb);
  int tok_bits;
  const int my = png_excl_sum(fb.bits, sh.scan, tok_bits);    // (the barriers inside also order the zeroing before the ORs)
  {
    PngEmit fe{sh.code};
    fe.out.begin(words, nwords, (long long)sh.hdr_bits + my);
    png_walk(s_bytes, c0, c1, prev_head, next_head, fe);
    fe.out.end();
  }
  if (tid == 64) {                 // the header (a lane of another wave than lane 0's, which has just done the serial part)
    PngOut o;
    o.begin(words, nwords, 0);
    o.put(last ? 1u : 0u, 1); o.put(2u, 2);
    o.put((unsigned)(sh.hlit - 257), 5); o.put(1u, 5); o.put((unsigned)(sh.hclen - 4), 4);
    for (int k = 0; k < sh.hclen; k++) o.put(sh.cl_lens[c_cl_order[k]], 3);
    for (int t = 0; t < sh.n_cltok; t++) {
      const int s = sh.cl_sym[t];
      const unsigned c = sh.cl_code[s];
      o.put(c & 0xffffu, (int)(c >> 16));
      if (s >= 16) o.put(sh.cl_ext[t], s == 16 ? 2 : s == 17 ? 3 : 7);
    }
    o.end();
  }
  if (tid == 128) {                // end of block and, behind every strip but the last, the sync flush
    PngOut o;
    o.begin(words, nwords, (long long)sh.hdr_bits + tok_bits);
    const unsigned c = sh.code[256];
    o.put(c & 0xffffu, (int)(c >> 16));
    if (!last) { o.put(0u, 3); o.align(); o.put(0xffff0000u, 32); }
    o.end();
  }
}

// ---- compaction --------------------------------------------------------------------------------------------------------------------------
struct PngGather {
  const uint8_t *slots; size_t slot_stride;
  const int32_t *sizes, *kinds, *start;       // start: exclusive scan of sizes over all strips of the batch, [n S + 1]
  const unsigned *adler_a, *adler_b;
  int n, H, row, strip_rows, S;
  uint8_t *out; long long *offsets; int32_t *n_stored, *strip_kinds;
};
__global__ __launch_bounds__(256) void k_png_gather(PngGather G) {
  __shared__ int s_w[4];
  const int strip = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
  const size_t sidx = (size_t)img * G.S + strip;
  const uint8_t *src = G.slots + sidx * G.slot_stride;
  const int size = G.sizes[sidx];
  const long long at = (long long)G.start[(size_t)img * G.S] + 6ll * img;      // the stream's first byte
  uint8_t *dst = G.out + (long long)G.start[sidx] + 6ll * img + 2;
  for (int i = tid; i < size; i += 256) dst[i] = src[i];
  if (G.strip_kinds && tid == 0) G.strip_kinds[sidx] = G.kinds[sidx];
  if (strip == 0 && tid == 0) {
    G.out[at] = 0x78; G.out[at + 1] = 0x01;
    G.offsets[img] = at;
    if (img == G.n - 1) G.offsets[G.n] = (long long)G.start[(size_t)G.n * G.S] + 6ll * G.n;
  }
  if (strip == G.S - 1 && tid == 0) {          // the Adler-32 of the image from its strips' sums, in strip order.  Loop: S strips
    u64 a = 1, b = 0;
    for (int k = 0; k < G.S; k++) {
      const size_t q = (size_t)img * G.S + k;
      const u64 Lk = (u64)min(G.strip_rows, G.H - k * G.strip_rows) * G.row;
      b = (b + (Lk % PNG_ADLER) * a + G.adler_b[q]) % PNG_ADLER;
      a = (a + G.adler_a[q]) % PNG_ADLER;
    }
    uint8_t *t = dst + size;
    t[0] = (uint8_t)(b >> 8); t[1] = (uint8_t)(b & 255); t[2] = (uint8_t)(a >> 8); t[3] = (uint8_t)(a & 255);
  }
  if (strip == 0 && img == 0) {                // the stored strips of the batch.  Loop: n S / 256 trips
    int c = 0;
    for (long long q = tid; q < (long long)G.n * G.S; q += 256) c += G.kinds[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((tid & 63) == 0) s_w[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) *G.n_stored = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  }
}

struct PngLayout { int S; long long per_image; size_t slot_stride, slots, sizes, kinds, adler_a, adler_b, start, bsum, total; };

// the one place sizes are derived: strips, the bound and the workspace
bool png_layout(int n, int H, int W, int C, int strip_rows, PngLayout *P) {
  if (n < 1 || n > IA_PNG_MAX_IMAGES || H < 1 || W < 1 || (C != 3 && C != 4) || strip_rows < 1) return false;
  const long long row = (long long)W * C + 1;
  const long long sr = strip_rows < H ? strip_rows : H;
  if (sr * row > IA_PNG_MAX_STRIP_BYTES) return false;
  const long long full = H / sr, rest = H % sr;
  const long long S = full + (rest ? 1 : 0);
  P->per_image = 6 + full * png_stored_bytes_host(sr * row) + (rest ? png_stored_bytes_host(rest * row) : 0);
  if (P->per_image * n >= (1ll << 31) || S * n >= (1ll << 31)) return false;
  P->S = (int)S;
  const size_t ns = (size_t)n * S;
  P->slot_stride = ia_align((size_t)png_stored_bytes_host(sr * row) + 4);
  size_t off = 0;
  P->slots = off; off += ns * P->slot_stride;
  P->sizes = off; off += ia_align(ns * 4);
  P->kinds = off; off += ia_align(ns * 4);
  P->adler_a = off; off += ia_align(ns * 4);
  P->adler_b = off; off += ia_align(ns * 4);
  P->start = off; off += ia_align((ns + 1) * 4);
  P->bsum = off; off += ia_align((size_t)ia_div_up((long)ns, IA_SCAN_THREADS) * 4);
  P->total = off;
  return true;
}

}  // namespace

extern "C" int ia_png_strips(int H, int W, int C, int strip_rows) {
  PngLayout P;
  return png_layout(1, H, W, C, strip_rows, &P) ? P.S : 0;
}

extern "C" size_t ia_png_bound_bytes(int n, int H, int W, int C, int strip_rows) {
  PngLayout P;
  return png_layout(n, H, W, C, strip_rows, &P) ? (size_t)(P.per_image * n) : 0;
}

extern "C" size_t ia_png_workspace_bytes(int n, int H, int W, int C, int strip_rows) {
  PngLayout P;
  return png_layout(n, H, W, C, strip_rows, &P) ? P.total : 0;
}

extern "C" int ia_png_encode(const uint8_t *images, int n, int H, int W, int C, int swap_rb, int strip_rows, uint8_t *out, size_t out_bytes,
                             long long *offsets, int32_t *n_stored, int32_t *strip_kinds, void *ws, size_t ws_bytes, void *stream) {
  IA_CHECK_ARG(n >= 0, "ia_png_encode: n < 0");
  if (n == 0) return IA_OK;
  IA_CHECK_ARG(stream != nullptr, "ia_png_encode: an explicit stream is required (stream = NULL)");
  IA_CHECK_ARG(C == 3 || C == 4, "ia_png_encode: C = %d: 3 (RGB) or 4 (RGBA)", C);
  IA_CHECK_ARG(strip_rows >= 1, "ia_png_encode: strip_rows %d < 1", strip_rows);
  PngLayout P;
  IA_CHECK_ARG(png_layout(n, H, W, C, strip_rows, &P),
               "ia_png_encode: %d images of %d x %d x %d in strips of %d rows: outside 1 <= n <= %d, H, W >= 1, a strip of at most %d "
               "filtered bytes, less than 2^31 bytes in all", n, H, W, C, strip_rows, IA_PNG_MAX_IMAGES, IA_PNG_MAX_STRIP_BYTES);
  IA_CHECK_ARG(images && out && offsets && n_stored, "ia_png_encode: images, out, offsets and n_stored are required");
  const size_t bound = (size_t)(P.per_image * n);
  IA_CHECK_ARG(out_bytes >= bound, "ia_png_encode: out of %zu bytes, %zu needed (ia_png_bound_bytes)", out_bytes, bound);
  IA_CHECK_ARG(ws && ws_bytes >= P.total, "ia_png_encode: workspace of %zu bytes, %zu needed (ia_png_workspace_bytes)",
               ws ? ws_bytes : (size_t)0, P.total);
  IA_CHECK_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)offsets & 7) == 0 && ((uintptr_t)n_stored & 3) == 0 &&
               (!strip_kinds || ((uintptr_t)strip_kinds & 3) == 0),
               "ia_png_encode: ws must be 16-byte aligned, offsets 8-byte, n_stored / strip_kinds 4-byte aligned");
  const hipStream_t s = (hipStream_t)stream;
  char *b = (char *)ws;
  const int sr = strip_rows < H ? strip_rows : H;
  const size_t lds = ((size_t)sr * ((size_t)W * C + 1) + 15) & ~(size_t)15;
  PngArgs A;
  A.images = images; A.H = H; A.W = W; A.strip_rows = sr; A.swap_rb = swap_rb; A.S = P.S;
  A.slots = (uint8_t *)(b + P.slots); A.slot_stride = P.slot_stride;
  A.sizes = (int32_t *)(b + P.sizes); A.kinds = (int32_t *)(b + P.kinds);
  A.adler_a = (unsigned *)(b + P.adler_a); A.adler_b = (unsigned *)(b + P.adler_b);
  if (lds + sizeof(PngShared) > 48 * 1024) {         // more LDS than a kernel gets unasked (on the current device)
    const void *k = C == 3 ? reinterpret_cast<const void *>(&k_png_strip<3>) : reinterpret_cast<const void *>(&k_png_strip<4>);
    (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, IA_PNG_MAX_STRIP_BYTES + 16);
  }
  const dim3 grid(P.S, n);
  if (C == 3) hipLaunchKernelGGL(k_png_strip<3>, grid, dim3(PNG_THREADS), lds, s, A);
  else hipLaunchKernelGGL(k_png_strip<4>, grid, dim3(PNG_THREADS), lds, s, A);
  IA_LAUNCH_CHECK("k_png_strip");
  const long long ns = (long long)n * P.S;
  int32_t *start = (int32_t *)(b + P.start);
  ia_scan(LoadInt{A.sizes}, ns, (int32_t *)(b + P.bsum), start, (int32_t *)nullptr, s);
  IA_LAUNCH_CHECK("ia_scan");
  PngGather G;
  G.slots = A.slots; G.slot_stride = P.slot_stride; G.sizes = A.sizes; G.kinds = A.kinds; G.start = start;
  G.adler_a = A.adler_a; G.adler_b = A.adler_b;
  G.n = n; G.H = H; G.row = W * C + 1; G.strip_rows = sr; G.S = P.S;
  G.out = out; G.offsets = offsets; G.n_stored = n_stored; G.strip_kinds = strip_kinds;
  hipLaunchKernelGGL(k_png_gather, grid, dim3(256), 0, s, G);
  IA_LAUNCH_CHECK("k_png_gather");
  return IA_OK;
}
