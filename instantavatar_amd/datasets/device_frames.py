"""The data side of a training step on the device: what
instant_avatar/datasets/peoplesnapshot.py does per item on the host with numpy / cv2 in 8 DataLoader workers --
camera rays (:12-25), masked compositing with a random background (:107-115), the sampler call (:117-119), near / far
(:141-150) -- with the frames resident in HBM and every step a handful of kernels.  At ~1.2 ms per training step the
host loader would be the bottleneck.

Image decoding and resizing (cv2.imread / cv2.resize, :100-105) happen once per sequence, in
`DeviceFrames.from_directory`: the files of a sequence directory (datasets/sequence_dir.py) are decoded with PIL on host
threads, staged chunk by chunk through pinned memory, and resized by `ia_io_ingest_chunk` (csrc/ia_io.hip) straight into
the resident stores -- the full-resolution sequence is never resident, on the device or on the host.  The factor-2
resize rule is PARITY UNPINNED against OpenCV itself (no cv2 to compare with); see sequence_dir.py.  `DeviceFrames.from_arrays` still takes arrays that are already decoded and at the training resolution.
"""
import concurrent.futures
import ctypes as C
import os
import time

import numpy as np
import torch

from .. import _lib
from ..utils.sampler import EdgeSampler, PatchSampler


def make_rays(K, c2w, H, W, device):
    """peoplesnapshot.py:17-25 on the device: (rays_o, rays_d) float32 [H, W, 3].  K [3,3], c2w [4,4] (or [3,4]): host arrays."""
    K = np.asarray(K, np.float64)
    c2w = np.asarray(c2w, np.float64)
    Kinv = np.ascontiguousarray(np.linalg.inv(K))
    R = np.ascontiguousarray(c2w[:3, :3])
    t = np.ascontiguousarray(c2w[:3, 3])
    o = torch.empty((H, W, 3), device=device)
    d = torch.empty((H, W, 3), device=device)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    _lib.require_cuda(o)
    _lib.call("ia_make_rays", dp(Kinv), dp(R), dp(t), H, W, o, d)
    return o, d


_MASK_FORMS = {"peoplesnapshot": 1, "custom": 2}     # IA_IO_MASK_U8 / IA_IO_MASK_GREY (include/instantavatar_hip_io.h)


def _decode_image(path, out):
    """cv2.imread(path) into out uint8 [H0, W0, 3]: three channels B, G, R, an alpha channel dropped, grey replicated"""
    from PIL import Image
    from .sequence_dir import SequenceError
    with Image.open(path) as im:
        if im.mode not in ("RGB", "RGBA", "L", "P"):
            raise SequenceError("%s: PNG mode %s (more than 8 bits per channel?) is not read here; cv2.imread would convert it" % (path, im.mode))
        a = np.asarray(im.convert("RGB"))
    if a.shape != out.shape:
        raise SequenceError("%s is %d x %d, expected %d x %d" % (path, a.shape[0], a.shape[1], out.shape[0], out.shape[1]))
    out[...] = a[..., ::-1]


def _decode_mask(path, out, kind):
    """the mask file's bytes into out uint8 [H0, W0]: np.load (peoplesnapshot.py:101) or cv2.imread(path, IMREAD_GRAYSCALE)
    (custom.py:99; its `/ 255` is the kernel's)"""
    from .sequence_dir import SequenceError
    if kind == "peoplesnapshot":
        a = np.load(path)
        if a.dtype != np.uint8:
            raise SequenceError("%s: a %s mask; the reference's preprocessing writes uint8 0/1 arrays, and cv2.resize of another "
                                "type follows another rule" % (path, a.dtype))
    else:
        from PIL import Image
        with Image.open(path) as im:
            if im.mode != "L":
                raise SequenceError("%s: PNG mode %s; a mask is an 8-bit grey image (cv2's colour -> grey conversion is not restated)" % (path, im.mode))
            a = np.asarray(im)
    if a.shape != out.shape:
        raise SequenceError("%s has shape %s, expected %s" % (path, a.shape, out.shape))
    out[...] = a


class DeviceFrames:
    """A sequence's frames, masks, camera rays and SMPL parameters resident on the GPU; `batch(idx)` is
    PeopleSnapshotDataset.__getitem__ for split == "train" (peoplesnapshot.py:99-151) followed by the DataLoader's
    batch dimension of 1."""

    def __init__(self, images_u8, masks, K, c2w, smpl_params, sampler, near=None, far=None):
        """images_u8: uint8 [N,H,W,3] (as cv2.imread returns them, already at the training resolution);
        masks: float [N,H,W]; smpl_params: dict of arrays (betas [1,10], body_pose [N,69], global_orient [N,3], transl [N,3])."""
        self.images = images_u8
        self.masks = masks
        _lib.require_cuda(images_u8, masks)
        N, H, W, _ = images_u8.shape
        self.N, self.H, self.W = N, H, W
        self.K, self.c2w = np.asarray(K, np.float64).copy(), np.asarray(c2w, np.float64).copy()      # host copies: `camera()`
        self.rays_o, self.rays_d = make_rays(K, c2w, H, W, images_u8.device)
        dev = images_u8.device
        self.smpl_params = {k: torch.as_tensor(np.asarray(v, np.float32), device=dev) for k, v in smpl_params.items()}
        go, bp = self.smpl_params.get("global_orient"), self.smpl_params.get("body_pose")
        if go is not None and bp is not None and go.dim() == 2 and bp.dim() == 2 and go.shape[1] == 3 and bp.shape[1] == 69 and go.shape[0] == bp.shape[0]:
            # the two pose tables as column ranges of ONE [N, 72] table: a frame's (global_orient, body_pose) pair is one contiguous
            # 72-float record then, which prepare_deformer hands to ia_smpl_tfs in place (snarf_deformer._pose72: no concatenation launch)
            pose72 = torch.cat([go, bp], dim=1).contiguous()
            self.smpl_params["global_orient"], self.smpl_params["body_pose"] = pose72[:, :3], pose72[:, 3:]
        self.sampler = sampler
        self.near, self.far = near, far
        self._idx_all = torch.arange(N, device=dev)   # `idx_dev` of a batch is a one-element view: no host -> device copy per step

    @classmethod
    def from_arrays(cls, images_u8, masks, K, c2w, smpl_params, sampler, device, **kw):
        return cls(torch.as_tensor(np.ascontiguousarray(images_u8), device=device), torch.as_tensor(np.ascontiguousarray(masks, np.float32), device=device),
                   K, c2w, smpl_params, sampler, **kw)

    @classmethod
    def from_directory(cls, seq, sampler, device, chunk=None, workers=None, log=None):
        """The frames of `seq` (sequence_dir.read_sequence) decoded, resized by seq.downscale and resident on `device`.
        chunk: frames per staged chunk (default: about 32 MB of full-resolution pixels); workers: decoding threads, at most
        min(16, os.cpu_count()); log: a callable that is handed the one-line report of the load (frames, seconds, MB/s decoded).
        Three stages overlap on consecutive chunks: PIL decodes chunk k + 1 into one pinned buffer while the side stream
        copies chunk k from the other and `ia_io_ingest_chunk` writes its frames into the stores."""
        from .sequence_dir import resize_rule
        factor = resize_rule(seq.H0, seq.W0, seq.downscale)
        if (seq.H, seq.W) != (seq.H0 // factor, seq.W0 // factor):
            raise ValueError("sequence: training size %d x %d is not the source size %d x %d over %d" % (seq.H, seq.W, seq.H0, seq.W0, factor))
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.IAError("DeviceFrames.from_directory needs a GPU device (got %s); there is no CPU path" % device)
        N, H0, W0, H, W = len(seq.image_files), seq.H0, seq.W0, seq.H, seq.W
        px = H0 * W0
        chunk = max(1, min(N, int(chunk) if chunk else (32 << 20) // (px * 4) or 1))
        workers = max(1, min(16, os.cpu_count() or 1, int(workers) if workers else 16))
        form = _MASK_FORMS[seq.kind]
        t0 = time.perf_counter()
        with torch.cuda.device(device):
            images = torch.empty((N, H, W, 3), dtype=torch.uint8, device=device)
            masks = torch.empty((N, H, W), dtype=torch.float32, device=device)
            # per slot: [chunk, H0, W0, 3] image bytes followed by [chunk, H0, W0] mask bytes -- one copy per chunk
            host = [torch.empty(chunk * px * 4, dtype=torch.uint8).pin_memory() for _ in range(2)]
            dev = [torch.empty(chunk * px * 4, dtype=torch.uint8, device=device) for _ in range(2)]
            copied = [None, None]         # per slot: the event after the last copy out of its pinned buffer
            side = torch.cuda.Stream(device)
            with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
                for k, first in enumerate(range(0, N, chunk)):
                    n, slot = min(chunk, N - first), k % 2
                    if copied[slot] is not None:
                        copied[slot].synchronize()      # the pinned buffer is free again (chunk k - 2 has left it)
                    h = host[slot].numpy()
                    h_img, h_msk = h[:chunk * px * 3].reshape(chunk, H0, W0, 3), h[chunk * px * 3:].reshape(chunk, H0, W0)
                    jobs = [pool.submit(_decode_image, seq.image_files[first + i], h_img[i]) for i in range(n)]
                    jobs += [pool.submit(_decode_mask, seq.mask_files[first + i], h_msk[i], seq.kind) for i in range(n)]
                    for j in jobs:
                        j.result()
                    with torch.cuda.stream(side):
                        # (the device staging buffer of the slot is reused in stream order behind chunk k - 2's kernel)
                        dev[slot].copy_(host[slot], non_blocking=True)
                        copied[slot] = torch.cuda.Event()
                        copied[slot].record(side)
                        d = dev[slot]
                        _lib.call("ia_io_ingest_chunk", d[:chunk * px * 3], d[chunk * px * 3:], form, n, H0, W0, factor, images, masks, first, N)
            side.synchronize()
        dt = time.perf_counter() - t0
        if log is not None:
            mb = N * px * 4 / 1e6
            log("loaded %d frames %dx%d -> %dx%d (%s, downscale %d) in %.2f s: %.1f MB/s decoded, %d decoding threads, chunks of %d" % (
                N, W0, H0, W, H, seq.kind, factor, dt, mb / max(dt, 1e-9), workers, chunk))
        return cls(images, masks, seq.K, seq.c2w, seq.smpl_params, sampler, near=seq.near, far=seq.far)

    def __len__(self):
        return self.N

    def camera(self, near=0.05):
        """the sequence's camera for the mesh rasteriser (`raster.Camera`): its K, w2c = c2w^-1 on the device, its image size -- the
        camera its rays were made from, so a raster frame of a posed mesh overlays the frame's image"""
        from ..raster import Camera
        c2w = np.eye(4)
        c2w[:self.c2w.shape[0], :] = self.c2w                      # ([3,4] or [4,4])
        w2c = torch.as_tensor(np.linalg.inv(c2w), dtype=torch.float32, device=self.images.device)
        return Camera(self.K, w2c, self.H, self.W, near=near)

    def frame(self, idx):
        """PeopleSnapshotDataset.__getitem__ for split "val" / "test" (peoplesnapshot.py:112-125): the WHOLE frame, white
        background, rays / rgb / alpha flattened to [1, H*W, ...] -- what validation_step hands to render_image_fast."""
        dev = self.images.device
        H, W = self.H, self.W
        n = H * W
        if getattr(self, "_all_pixels", None) is None:
            self._all_pixels = torch.arange(n, dtype=torch.int32, device=dev)
        rgb, alpha = torch.empty((n, 3), device=dev), torch.empty(n, device=dev)
        ro, rd = torch.empty((n, 3), device=dev), torch.empty((n, 3), device=dev)
        bg = torch.empty((n, 3), device=dev)
        img = self.images[idx]
        img_u8 = img if img.dtype == torch.uint8 else None
        img_f = None if img_u8 is not None else img.float().contiguous()
        m = self.masks[idx].float().contiguous()
        _lib.call("ia_sample_batch", img_u8, img_f, m, self.rays_o, self.rays_d, H, W, self._all_pixels, None, None, 0, 0, n, None, rgb,
                  alpha, ro, rd, bg, None)   # bg NULL = white (:114)
        p = self.smpl_params
        transl = p["transl"][idx]
        near, far = torch.empty(n, device=dev), torch.empty(n, device=dev)
        if self.near is not None and self.far is not None:
            near.fill_(float(self.near))
            far.fill_(float(self.far))
        else:
            _lib.call("ia_near_far", transl.contiguous(), n, near, far)
        return {"rgb": rgb[None], "rays_o": ro[None], "rays_d": rd[None], "betas": p["betas"][0][None],
                "global_orient": p["global_orient"][idx][None], "body_pose": p["body_pose"][idx][None], "transl": transl[None],
                "alpha": alpha[None], "bg_color": bg.reshape(1, H, W, 3),   # the reference leaves bg_color un-flattened (:114)
                "idx": torch.tensor([idx]), "near": near[None], "far": far[None]}

    def batch(self, idx, draws=None, bg_draws=None, generator=None, out=None):
        """One training batch (leading batch dimension 1, as the reference's DataLoader with batch_size=1 yields).
        out: a batch dict returned by an earlier call (or `training.GraphedTrainStep.inputs`, the static input tensors of
        a captured step): the kernels write into its tensors instead of fresh ones -- no copies afterwards."""
        dev = self.images.device
        H, W = self.H, self.W
        mask2d = self.masks[idx]
        s = self.sampler
        flat_idx = rows = cols = None
        if isinstance(s, EdgeSampler):
            flat_idx = s.sample_indices(mask2d, draws=draws, generator=generator)
            n, shape, P, n_patch = flat_idx.numel(), (flat_idx.numel(),), 0, 0
        elif isinstance(s, PatchSampler):
            rows, cols = s.sample_corners(mask2d, draws=draws, generator=generator)
            P, n_patch = s.patch_size, s.n
            n, shape = n_patch * P * P, (n_patch, P, P)
        else:
            raise TypeError("DeviceFrames needs an instantavatar_amd.utils.sampler.EdgeSampler / PatchSampler")
        def dst(key, *shp):
            """the tensor results are written to: the caller's (if it has the right shape) or a fresh one"""
            t = out.get(key) if out is not None else None
            if torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == int(np.prod(shp)):
                return t.view(*shp)
            return torch.empty(shp, device=dev)

        bg = dst("bg_color", n, 3)
        if bg_draws is None:
            bg.uniform_(0.0, 1.0, generator=generator)                       # np.random.rand(*img.shape) at :111, for the sampled pixels
        else:
            bg.copy_(bg_draws.reshape(n, 3))
        rgb, alpha = dst("rgb", n, 3), dst("alpha", n)
        ro, rd = dst("rays_o", n, 3), dst("rays_d", n, 3)
        img = self.images[idx]
        img_u8 = img if img.dtype == torch.uint8 else None
        img_f = None if img_u8 is not None else img.float().contiguous()
        m = mask2d.float().contiguous()
        _lib.call("ia_sample_batch", img_u8, img_f, m, self.rays_o, self.rays_d, H, W, flat_idx, rows, cols, n_patch, P, n, bg, rgb, alpha,
                  ro, rd, None, None)
        p = self.smpl_params
        transl = p["transl"][idx]
        near, far = dst("near", n), dst("far", n)
        if self.near is not None and self.far is not None:
            near.fill_(float(self.near))
            far.fill_(float(self.far))
        else:  # distance from the camera to the mid-hip (:146-150), one launch
            _lib.call("ia_near_far", transl.contiguous(), n, near, far)
        res = {
            "rgb": rgb.reshape(1, *shape, 3), "rays_o": ro.reshape(1, *shape, 3), "rays_d": rd.reshape(1, *shape, 3),
            "betas": p["betas"][0][None], "global_orient": p["global_orient"][idx][None], "body_pose": p["body_pose"][idx][None],
            "transl": transl[None], "alpha": alpha.reshape(1, *shape), "bg_color": bg.reshape(1, *shape, 3),
            "idx": torch.tensor([idx]),   # host tensor: the trainer reads it as a Python int (renderer.idx) without a device sync
            "idx_dev": self._idx_all[idx:idx + 1],   # the same index on the device: row of the SMPLParamEmbedding tables (DNeRF.py:114)
            "near": near.reshape(1, *shape), "far": far.reshape(1, *shape),
        }
        if out is not None:
            # SMPL parameters of the frame into the caller's tensors too; what was written in place is returned as the
            # caller's own tensor objects, so that `batch is out`-style identity checks downstream see no copy to make
            dsts, srcs = [], []
            for k in ("betas", "global_orient", "body_pose", "transl", "idx_dev"):
                t = out.get(k)
                if torch.is_tensor(t) and t.is_cuda and t.shape == res[k].shape:
                    if t.dtype == torch.float32 and res[k].dtype == torch.float32:
                        dsts.append(t)
                        srcs.append(res[k])
                    else:
                        t.copy_(res[k], non_blocking=True)
                    res[k] = t
            if dsts:
                torch._foreach_copy_(dsts, srcs, non_blocking=True)   # the four SMPL vectors in ONE launch (was four ~5 us copies)
            for k in ("rgb", "rays_o", "rays_d", "alpha", "bg_color", "near", "far"):
                t = out.get(k)
                if torch.is_tensor(t) and t.data_ptr() == res[k].data_ptr() and t.shape == res[k].shape:
                    res[k] = t
        return res
