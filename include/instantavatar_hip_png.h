/*
 * instantavatar_hip_png.h -- encoding a batch of rendered 8-bit frames on the device: PNG filtering and deflate, so that only compressed
 * bytes cross to the host (csrc/ia_png.hip).  The result of a call is n complete zlib streams -- exactly the payload of a PNG's IDAT
 * chunk -- compacted into one device buffer; signature, IHDR, chunk lengths and CRCs are framed on the host (instantavatar_amd/png.py).
 * Conventions as in instantavatar_hip.h (device pointers, `stream` as void* and never NULL here, no allocation, scratch through `ws`,
 * 0 = IA_OK, no host synchronisation, on a bad argument nothing is written); a header of its own, bound by `_lib` as a twentieth table.
 *
 * Definition ("PNG encoding"), all of it integer arithmetic.  The bytes of image i are a function of its pixels, C,
 * swap_rb and strip_rows and of nothing else: not of n, of i, of the launch geometry or of the order of any atomic operation.
 *   pixels      images [n,H,W,C] uint8, C = 3 (colour type 2) or 4 (colour type 6).  swap_rb != 0 exchanges channels 0 and 2 while reading.
 *   filter      row y becomes 1 + W C bytes: the filter type, then the filtered bytes of that type (PNG's None 0, Sub 1, Up 2, Average 3,
 *               Paeth 4, bpp = C).  The type is the one with the smallest sum of |filtered byte read as int8|; a tie goes to the lower
 *               type.  The row above row 0 of an image is zero; every other row, a strip's first included, is filtered against the raw
 *               row above it.
 *   strips      rows [k strip_rows, min(H, (k + 1) strip_rows)) are strip k, S = ceil(H / strip_rows) of them; each is compressed on its
 *               own (one workgroup), its bytes being the filtered rows one after the other.  min(strip_rows, H) (W C + 1) may not exceed
 *               IA_PNG_MAX_STRIP_BYTES (the strip is held in LDS: 124 KiB of the CU's 160 KiB; tokens are never stored, they are recomputed
 *               from the bytes).  IA_PNG_DEFAULT_STRIP_ROWS = 16 fits rows of up to 1920 x 4 bytes.
 *   tokens      literals and matches of distance 1 only, none reaching back before the strip's first byte.  A maximal run of m + 1 equal
 *               bytes is one literal, then floor(m / 258) matches of length 258, then the remainder r = m mod 258 as one match of length r
 *               if r >= 3 and as r literals otherwise.
 *   codes       one dynamic-Huffman block (BTYPE 2) per strip.  Literal/length frequencies are the strip's own histogram plus one
 *               end-of-block; HLIT reaches to the last used symbol (at least 257).  The distance alphabet is always the two codes 0 and
 *               1 of one bit each (HDIST = 2), a match costs the one bit 0.  Code lengths of an alphabet, limit 15 bits (7 for the
 *               code-length code):
 *                 order  the used symbols ascending by (frequency, symbol)
 *                 merge  Huffman's algorithm on two queues (leaves in that order, merged nodes in the order they are made); of a leaf and
 *                        a merged node of equal weight the leaf is taken first
 *                 limit  c[d] = leaves at depth d, depths above the limit counted at the limit; while the Kraft sum, in units of
 *                        2^-limit, exceeds 2^limit: c[limit] -= 1; for the largest d < limit with c[d] > 0: c[d] -= 1, c[d + 1] += 2
 *                 hand   lengths 1, 2, ... are handed out from the END of the order: c[1] symbols get 1 bit, the next c[2] get 2, ...
 *               so the Kraft sum is exactly 1.  Codes are the canonical ones of RFC 1951 3.2.2.  The code lengths of both alphabets form
 *               one sequence (HLIT lengths, then 1, 1); a maximal run of k equal values v in it is coded as: v = 0: while k >= 11 one
 *               symbol 18 covering min(k, 138); then one symbol 17 if k >= 3, else k symbols 0.  v > 0: v once, then while k >= 3 one
 *               symbol 16 covering min(k, 6), then the remaining k (0 .. 2) times v.  HCLEN reaches to the last used symbol in the
 *               order 16, 17, 18, 0, 8, 7, ... (at least 4).
 *   strip end   the last strip of an image has BFINAL = 1.  Every other strip is followed by the empty stored block of a sync flush:
 *               three zero bits, zero bits up to the byte boundary, 00 00 FF FF -- it ends on a byte boundary with BFINAL 0.
 *   fallback    a strip of L bytes whose coded form (the sync flush included) is LONGER than L + 5 ceil(L / 65535) bytes is written as
 *               stored blocks of at most 65 535 bytes each instead (BFINAL on the last block of the last strip; no sync flush behind
 *               them, they end on a byte boundary anyway).  A stream is therefore never longer than ia_png_bound_bytes / n.
 *   stream      78 01, the strips, the Adler-32 (big endian) of all filtered bytes of the image, combined from per-strip sums
 *               A = sum b[i], B = sum (L - i) b[i] (mod 65521) by a' = a + A, b' = b + L a + B starting from a = 1, b = 0.
 *
 * ia_png_strips: S; 0 on arguments ia_png_encode refuses.
 * ia_png_bound_bytes: the size of `out` that ia_png_encode asks for = n (6 + sum over strips of L + 5 ceil(L / 65535)); 0 on arguments
 *   that ia_png_encode refuses (C not 3 or 4, H, W or strip_rows < 1, n < 1 or > IA_PNG_MAX_IMAGES, a strip above IA_PNG_MAX_STRIP_BYTES,
 *   a bound of 2^31 bytes or more).
 * ia_png_workspace_bytes: scratch of ia_png_encode (every strip's bytes before compaction, their sizes and sums); 0 likewise.
 * ia_png_encode: images [n,H,W,C] uint8 -> out: stream i at bytes [offsets[i], offsets[i + 1]) (offsets [n + 1] int64, offsets[0] = 0);
 *   n_stored [1] int32: strips of the batch that took the stored fallback; strip_kinds [n,S] int32 or NULL: 1 = stored, 0 = dynamic.
 *   out_bytes >= ia_png_bound_bytes, ws_bytes >= ia_png_workspace_bytes, ws 16-byte aligned.  Bytes of `out` behind offsets[n] are
 *   not written.  A fixed number of launches whatever n is; nothing has to be zeroed by the caller or survive in ws between calls. */
#ifndef INSTANTAVATAR_HIP_PNG_H
#define INSTANTAVATAR_HIP_PNG_H

#include "instantavatar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IA_PNG_DEFAULT_STRIP_ROWS 16
#define IA_PNG_MAX_STRIP_BYTES 126976
#define IA_PNG_MAX_IMAGES 65535
int ia_png_strips(int H, int W, int C, int strip_rows);
size_t ia_png_bound_bytes(int n, int H, int W, int C, int strip_rows);
size_t ia_png_workspace_bytes(int n, int H, int W, int C, int strip_rows);
int ia_png_encode(const uint8_t *images, int n, int H, int W, int C, int swap_rb, int strip_rows, uint8_t *out, size_t out_bytes,
                  long long *offsets, int32_t *n_stored, int32_t *strip_kinds, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_PNG_H */
