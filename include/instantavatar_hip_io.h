/*
 * instantavatar_hip_io.h -- the sequence-ingest part of the C ABI of libinstantavatar_hip.so (MI355X / gfx950).
 *
 * A header of its own next to instantavatar_hip.h (whose conventions hold here: device pointers owned by the caller,
 * `stream` a hipStream_t passed as void*, no synchronisation, no allocation, 0 = IA_OK / negative = error with
 * ia_last_error()).  The binding parses it with the same parser into a table of its own (`_lib.io_declarations()`),
 * so the main header's set of prototypes stays what it is.
 */
#ifndef INSTANTAVATAR_HIP_IO_H
#define INSTANTAVATAR_HIP_IO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* what a source mask byte stands for */
#define IA_IO_MASK_U8 1   /* the value itself (PeopleSnapshot: np.load of a uint8 0/1 array, peoplesnapshot.py:101)    */
#define IA_IO_MASK_GREY 2 /* float64 v / 255 (custom: cv2.imread(..., IMREAD_GRAYSCALE) / 255, custom.py:99)           */

/* One chunk of decoded full-resolution frames -> the resident stores of datasets.DeviceFrames, what
 * instant_avatar/datasets/peoplesnapshot.py:100-107 and custom.py:98-105 do per item with cv2.resize and astype:
 *   src_images  uint8 [n, H0, W0, 3] (as cv2.imread returns them) or NULL: no images in this launch
 *   src_masks   uint8 [n, H0, W0] or NULL: no masks in this launch; `mask_form` says what a byte stands for
 *   images      uint8 [n_frames, H0 / factor, W0 / factor, 3],  masks float32 [n_frames, H0 / factor, W0 / factor]:
 *               frame i of the chunk is written at frame first + i (first >= 0, first + n <= n_frames)
 * factor 1: a copy; masks = float32(v) (IA_IO_MASK_U8) or float32(v / 255.0), the division in float64 (IA_IO_MASK_GREY).
 * factor 2 (H0 and W0 even): the 2 x 2 box, a b the upper row and c d the lower one:
 *   uint8 sources (images per channel, IA_IO_MASK_U8):  (a + b + c + d + 2) >> 2
 *   IA_IO_MASK_GREY:  float32(((a / 255 + b / 255) + (c / 255 + d / 255)) * 0.25), evaluated in float64 in that order
 * Any other factor, an odd source size at factor 2 and a NULL `stream` (the default stream) are refused.
 * One launch for the images and the masks of the chunk. */
int ia_io_ingest_chunk(const uint8_t *src_images, const uint8_t *src_masks, int mask_form, int n, int H0, int W0,
                       int factor, uint8_t *images, float *masks, long long first, long long n_frames, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_IO_H */
