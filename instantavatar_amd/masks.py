"""Cleaning raw per-frame segmentation masks on the GPU (csrc/ia_masks.hip, include/instantavatar_hip_masks.h; definition in
DESIGN.md section 4, "mask cleaning"): threshold, k x k box open and close, connected components, keep the largest -- what
scripts/custom/extract-largest-connected-components.py of the reference does per frame with cv2, here for a whole batch of frames in a
fixed number of launches.  `drivers/clean_masks.py` is the command line around it.  There is no CPU route."""
import collections

import torch

from . import _lib

#: masks [n,H,W] uint8 (255 on the kept component), area [n] int32 (its pixels; 0: the frame has no foreground), n_components [n] int32;
#: with return_stages also binary [n,H,W] uint8 (0 / 255 after threshold, open and close) and labels [n,H,W] int32 (0 = background,
#: otherwise 1 + the row-major index of the first pixel of the component), else None.  A [H,W] input gives [H,W] images and 0-d counts.
CleanedMasks = collections.namedtuple("CleanedMasks", "masks area n_components binary labels")


class _Scratch:
    """the owner `_lib.scratch` caches the workspace on: one per device, grown and never shrunk"""


_scratch = {}


def _owner(device):
    """the device's workspace owner and the side stream every launch of this module goes to: the entry points take no NULL stream
    (torch's default one), and with one stream per device the shared workspace is only ever used in stream order"""
    o = _scratch.get(device)
    if o is None:
        o = _scratch[device] = _Scratch()
        o.stream = torch.cuda.Stream(device)
    return o


class _side_stream:
    """with _side_stream(device): the side stream picks up after torch's current stream, and the current stream after the side stream
    at the end -- ordered on the device, no host synchronisation"""

    def __init__(self, device):
        self.side, self.cur = _owner(device).stream, torch.cuda.current_stream(device)
        self.ctx = torch.cuda.stream(self.side)

    def __enter__(self):
        self.side.wait_stream(self.cur)
        self.ctx.__enter__()

    def __exit__(self, *exc):
        self.ctx.__exit__(*exc)
        self.cur.wait_stream(self.side)


@torch.no_grad()
def clean_masks(src, threshold=0, kernel_size=5, connectivity=8, return_stages=False):
    """src: uint8 CUDA tensor [n,H,W] or [H,W] -> CleanedMasks.  Foreground is src > threshold; kernel_size odd in [1, 31] (1: no
    morphology); connectivity 8 or 4.  Everything stays on the device and nothing is read back."""
    if not torch.is_tensor(src):
        raise TypeError("clean_masks: src is a uint8 tensor on the GPU, got %s" % type(src).__name__)
    _lib.require_cuda(src)
    if src.dtype != torch.uint8 or src.dim() not in (2, 3):
        raise _lib.IAError("clean_masks: src is uint8 [n,H,W] or [H,W], got %s %s" % (src.dtype, tuple(src.shape)))
    single = src.dim() == 2
    s = (src[None] if single else src).contiguous()
    n, H, W = s.shape
    dev = s.device
    masks = torch.empty_like(s)
    area, n_comp = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    binary = torch.empty_like(s) if return_stages else None
    labels = torch.empty((n, H, W), dtype=torch.int32, device=dev) if return_stages else None
    if n:
        with torch.cuda.device(dev), _side_stream(dev):
            nb = int(_lib.call("ia_mask_clean_workspace_bytes", n, H, W))
            if nb == 0:
                raise _lib.IAError("clean_masks: %d frames of %d x %d: outside 1 <= n <= 65535, H, W >= 1, H * round_up(W, 64) < 2^31" % (n, H, W))
            ws = _lib.scratch(_owner(dev), "_mask_ws", nb, dev)
            _lib.call("ia_mask_clean", s, n, H, W, int(threshold), int(kernel_size), int(connectivity), masks, binary, labels, area, n_comp,
                      ws, ws.numel())
    if single:
        return CleanedMasks(masks[0], area[0], n_comp[0], None if binary is None else binary[0], None if labels is None else labels[0])
    return CleanedMasks(masks, area, n_comp, binary, labels)


@torch.no_grad()
def apply_masks(images, masks, out=None):
    """images uint8 [n,H,W,3] (or [H,W,3]), masks uint8 [n,H,W] (or [H,W]) -> images with every pixel outside the mask set to 0;
    out: None (a new tensor) or a contiguous tensor of the images' shape, which may be `images` itself."""
    _lib.require_cuda(images, masks, out)
    if images.dtype != torch.uint8 or masks.dtype != torch.uint8 or images.shape[-1] != 3 or tuple(images.shape[:-1]) != tuple(masks.shape) \
            or masks.dim() not in (2, 3):
        raise _lib.IAError("apply_masks: images uint8 [n,H,W,3] and masks uint8 [n,H,W], got %s %s and %s %s"
                           % (images.dtype, tuple(images.shape), masks.dtype, tuple(masks.shape)))
    if out is None:
        images = images.contiguous()
        out = torch.empty_like(images)
    elif out.shape != images.shape or out.dtype != torch.uint8 or not out.is_contiguous() or not images.is_contiguous():
        raise _lib.IAError("apply_masks: out is a contiguous uint8 tensor of the shape of (contiguous) images")
    masks = masks.contiguous()
    H, W = masks.shape[-2:]
    n = masks.numel() // max(H * W, 1)
    if masks.numel():
        with torch.cuda.device(images.device), _side_stream(images.device):
            _lib.call("ia_mask_apply", images, masks, n, H, W, out)
    return out
