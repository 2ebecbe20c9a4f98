"""A tiny sequence directory in the reference's layout (datasets/sequence_dir.py), written deterministically from a
seed -- a helper of tests/test_cpu_sequence_dir.py, tests/test_gpu_sequence_dir.py and tests/golden/make_sequence_dir_golden.py,
not a test.  Also the independent numpy restatement of the ingest rule the kernel is pinned to (`restate_*`)."""
import os

import numpy as np

N, H0, W0, SEED = 7, 24, 20, 11

#: (name, kind, split, options, cached pose files {name under poses/: rows}).  Every option set the golden records; the
#: cached files have as many rows as the split has frames (a cached file is not sliced).
CASES = [
    ("ps_fallback", "peoplesnapshot", "train", dict(start=0, end=6, downscale=1), {}),
    ("ps_slice", "peoplesnapshot", "train", dict(start=1, end=5, skip=2, downscale=1), {}),
    ("ps_anim", "peoplesnapshot", "train", dict(start=0, end=6, skip=2, downscale=1), {"anim_nerf_train": 4, "train": 4}),
    ("ps_split", "peoplesnapshot", "train", dict(start=0, end=6, skip=2, downscale=1), {"train": 4}),
    ("ps_refine", "peoplesnapshot", "test", dict(start=3, end=6, skip=1, downscale=1, refine=True), {"anim_nerf_test": 4, "test": 4}),
    ("ps_refine_missing", "peoplesnapshot", "test", dict(start=3, end=6, skip=1, downscale=1, refine=True), {"test": 4}),
    ("ps_val", "peoplesnapshot", "val", dict(start=2, end=2, skip=4, downscale=1, near=2.0, far=5.0), {}),
    ("cu_cached", "custom", "train", dict(start=0, end=6, skip=2, downscale=1), {"train": 4}),
    ("cu_fitting", "custom", "train", dict(start=0, end=6, skip=2, downscale=1, fitting=True), {"train": 4}),
    ("cu_val", "custom", "val", dict(start=4, end=4, downscale=1), {}),
]
VAL_CASES = ("ps_val", "cu_val")     # the cases whose frame 0 is recorded as a val-split __getitem__


def _poses(rs, rows, thetas):
    d = dict(betas=rs.randn(10) * 0.5, transl=rs.randn(rows, 3) * 0.2 + [0.0, 0.1, 3.5])     # float64 on disk: the loader casts
    pose = rs.randn(rows, 72) * 0.2
    if thetas:
        d["thetas"] = pose
    else:
        d["global_orient"], d["body_pose"] = pose[:, :3], pose[:, 3:]
    return d


def write_sequence(root, kind, cached=None, seed=SEED, n=N, height=H0, width=W0):
    """Writes the directory and returns what was written: images uint8 [n,H0,W0,3] in cv2.imread's channel order (B, G, R),
    the mask files' bytes uint8 [n,H0,W0], and the camera."""
    from PIL import Image
    root = os.fspath(root)
    rs = np.random.RandomState(seed)
    H, W = height, width
    images = rs.randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    masks = (rs.rand(n, H, W) < 0.5).astype(np.uint8)
    for i in range(n):
        for _ in range(4):                                  # blocks of equal values
            y, x = rs.randint(0, H - 4), rs.randint(0, W - 4)
            images[i, y:y + 4, x:x + 4] = rs.randint(0, 256, 3)
            masks[i, y:y + 4, x:x + 4] = rs.randint(0, 2)
        for _ in range(6):                                  # isolated extreme pixels
            images[i, rs.randint(0, H), rs.randint(0, W)] = rs.choice([0, 255], 3)
        # all five fill counts of a 2 x 2 cell, in the first row of cells
        for c, fill in enumerate(([0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 1, 0], [1, 1, 0, 1], [1, 1, 1, 1])):
            masks[i, 0:2, 2 * c:2 * c + 2] = np.array(fill, np.uint8).reshape(2, 2)
    if kind == "custom":
        masks = masks * np.uint8(255)
        soft = rs.rand(n, H, W) < 0.15                      # grey levels in between: the float64 v / 255 path
        masks[soft] = rs.randint(1, 255, int(soft.sum())).astype(np.uint8)
    os.makedirs(os.path.join(root, "images"))
    os.makedirs(os.path.join(root, "masks"))
    os.makedirs(os.path.join(root, "poses"))
    for i in range(n):
        Image.fromarray(np.ascontiguousarray(images[i, ..., ::-1]), "RGB").save(os.path.join(root, "images", "image_%04d.png" % i))
        if kind == "custom":
            Image.fromarray(masks[i], "L").save(os.path.join(root, "masks", "mask_%04d.png" % i))
        else:
            np.save(os.path.join(root, "masks", "mask_%04d.npy" % i), masks[i])
    K = np.array([[41.5, 0.0, W / 2 + 0.25], [0.0, 40.75, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    a, b = 0.3, -0.2
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    ext = np.eye(4)
    ext[:3, :3] = Ry @ Rx
    ext[:3, 3] = [0.1, -0.2, 0.3]
    np.savez(os.path.join(root, "cameras.npz"), intrinsic=K, extrinsic=ext, height=H, width=W)
    np.savez(os.path.join(root, "poses.npz"), **_poses(np.random.RandomState(seed + 1), n, thetas=True))
    if kind == "custom":
        np.savez(os.path.join(root, "poses_optimized.npz"), **_poses(np.random.RandomState(seed + 2), n, thetas=False))
    for j, (name, rows) in enumerate(sorted((cached or {}).items())):
        np.savez(os.path.join(root, "poses", name + ".npz"), **_poses(np.random.RandomState(seed + 10 + sum(map(ord, name))), rows, thetas=j % 2 == 0))
    return dict(images=images, mask_bytes=masks, K=K, extrinsic=ext)


# ---- the ingest rule, restated with numpy (integer / float64), independently of the kernel -----------------------------
def restate_u8(src, factor):
    """uint8 [..., H0, W0(, C)] -> the copy (factor 1) or the rounded 2 x 2 box (a + b + c + d + 2) >> 2 (factor 2); the two
    spatial axes are the first two after the leading frame axis"""
    if factor == 1:
        return src.copy()
    s = src.astype(np.int64)
    a, b, c, d = s[:, 0::2, 0::2], s[:, 0::2, 1::2], s[:, 1::2, 0::2], s[:, 1::2, 1::2]
    return ((a + b + c + d + 2) >> 2).astype(np.uint8)


def restate_mask(mask_bytes, kind, factor):
    """the float32 mask store from the mask files' bytes [n, H0, W0]"""
    if kind == "peoplesnapshot":
        return restate_u8(mask_bytes, factor).astype(np.float32)
    m = mask_bytes.astype(np.float64) / 255.0
    if factor == 1:
        return m.astype(np.float32)
    a, b, c, d = m[:, 0::2, 0::2], m[:, 0::2, 1::2], m[:, 1::2, 0::2], m[:, 1::2, 1::2]
    return (((a + b) + (c + d)) * 0.25).astype(np.float32)
