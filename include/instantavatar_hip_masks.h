/*
 * instantavatar_hip_masks.h -- cleaning a batch of raw per-frame segmentation masks: threshold, box open and close, connected
 * components, keep the largest (csrc/ia_masks.hip; the step scripts/custom/extract-largest-connected-components.py of the reference
 * does with cv2).  Conventions as in instantavatar_hip.h (device pointers, `stream` as void* and never NULL here, no allocation,
 * scratch through `ws`, 0 = IA_OK, no host synchronisation); a header of its own, bound by `_lib` as an eighth table.
 *
 * Definition ("mask cleaning"), all of it integer arithmetic:
 *   foreground  src > threshold, threshold in [0, 255] (the reference: 0)
 *   morphology  kernel_size k odd in [1, IA_MASK_MAX_KERNEL], the full k x k box anchored at its centre; k = 1: none.  open = erode then
 *               dilate, close = dilate then erode, open first.  In every pass pixels outside the image are ignored: erode takes them as
 *               foreground, dilate as background (cv2's default border value for morphology, the rule of ia_mask_edge)
 *   components  connectivity 8 or 4 on the result.  labels: 0 = background, otherwise 1 + the row-major index, within its frame, of the
 *               first pixel of the pixel's component -- unique and independent of scheduling
 *   kept        the component of the largest area; a tie goes to the smallest label (a stated choice: cv2's label order is an artefact
 *               of its scan).  A frame without foreground after morphology gives an all-zero mask, area 0 and n_components 0 (the
 *               reference script stops there)
 * Frames are independent; two calls, or the same frame at another position of a batch, give the same bytes.  Every output element
 * is written; nothing has to be zeroed by the caller and nothing has to survive in ws between calls.
 *
 * ia_mask_clean_workspace_bytes: scratch of ia_mask_clean; 0 outside 1 <= n <= IA_MASK_MAX_FRAMES, H, W >= 1, H * round_up(W, 64) < 2^31.
 * ia_mask_clean: src [n,H,W] uint8 -> masks [n,H,W] uint8 (255 on the kept component, 0 elsewhere), binary [n,H,W] uint8 or NULL (0 / 255
 *   after threshold, open and close), labels [n,H,W] int32 or NULL, area [n] int32 (pixels of the kept component), n_components [n] int32.
 *   No output may overlap src.  A fixed number of launches whatever n is.
 * ia_mask_apply: images [n,H,W,3] uint8, masks [n,H,W] uint8 -> out[p] = masks[p] ? images[p] : 0 per pixel p; out may BE images
 *   (the same pointer), not overlap it otherwise. */
#ifndef INSTANTAVATAR_HIP_MASKS_H
#define INSTANTAVATAR_HIP_MASKS_H

#include "instantavatar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IA_MASK_MAX_KERNEL 31
#define IA_MASK_MAX_FRAMES 65535
size_t ia_mask_clean_workspace_bytes(int n, int H, int W);
int ia_mask_clean(const uint8_t *src, int n, int H, int W, int threshold, int kernel_size, int connectivity, uint8_t *masks,
                  uint8_t *binary, int32_t *labels, int32_t *area, int32_t *n_components, void *ws, size_t ws_bytes, void *stream);
int ia_mask_apply(const uint8_t *images, const uint8_t *masks, int n, int H, int W, uint8_t *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_MASKS_H */
