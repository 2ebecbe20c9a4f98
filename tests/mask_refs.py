"""Pure-numpy restatement of the mask cleaner (include/instantavatar_hip_masks.h; DESIGN.md section 4, "mask cleaning"): the reference
of tests/test_gpu_masks.py and the host baseline of tools/time_masks.py.  Integers only, so every comparison is for equality.
tests/test_cpu_mask_refs.py checks it against scipy.ndimage and against cases written out by hand.

    threshold   src > threshold
    erode       AND over the k x k box, pixels outside the image ignored (= foreground)
    dilate      OR over the k x k box, pixels outside the image ignored (= background)
    binary      erode, dilate (open), dilate, erode (close): four passes, as the definition lists them
    labels      0 = background, otherwise 1 + the row-major index of the first pixel of the component; by iterated minimum
                propagation over the 8 or 4 neighbours (nothing in common with the run-based union-find of the kernels)
    kept        the largest area, a tie to the smallest label
"""
import numpy as np


def threshold(src, thr=0):
    return np.asarray(src) > thr


def _shift(a, dy, dx, fill):
    """out[y, x] = a[y + dy, x + dx], `fill` where that is outside the image"""
    H, W = a.shape
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if abs(dy) < H and abs(dx) < W:
        out[yd, xd] = a[ys, xs]
    return out


def _box(a, k, erode):
    if k % 2 != 1 or k < 1:
        raise ValueError("kernel size %r: odd and >= 1" % (k,))
    r = (k - 1) // 2
    a = np.asarray(a, bool)
    rows = a.copy()                       # separable: along x, then along y
    for d in range(1, r + 1):
        for s in (-d, d):
            t = _shift(a, 0, s, erode)
            rows = rows & t if erode else rows | t
    out = rows.copy()
    for d in range(1, r + 1):
        for s in (-d, d):
            t = _shift(rows, s, 0, erode)
            out = out & t if erode else out | t
    return out


def erode(a, k):
    return _box(a, k, True)


def dilate(a, k):
    return _box(a, k, False)


def open_close(fg, k):
    """[H,W] bool -> bool: open (erode, dilate) then close (dilate, erode) with the k x k box"""
    return erode(dilate(dilate(erode(fg, k), k), k), k)


_N8 = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
_N4 = [(-1, 0), (0, -1), (0, 1), (1, 0)]


def label(fg, connectivity=8):
    """[H,W] bool -> int32 labels: every foreground pixel starts with 1 + its own index and takes the minimum over its neighbours
    until nothing changes (at most as many rounds as the longest shortest path inside a component)"""
    if connectivity not in (4, 8):
        raise ValueError("connectivity %r: 8 or 4" % (connectivity,))
    fg = np.asarray(fg, bool)
    H, W = fg.shape
    big = np.int64(H) * W + 1
    lab = np.where(fg, np.arange(1, H * W + 1, dtype=np.int64).reshape(H, W), big)
    nb = _N8 if connectivity == 8 else _N4
    while True:
        new = lab
        for dy, dx in nb:
            new = np.minimum(new, _shift(lab, dy, dx, big))
        new = np.where(fg, new, big)
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(fg, lab, 0).astype(np.int32)


def largest(lab):
    """labels -> (mask uint8 0 / 255, area, number of components); the largest area, a tie to the smallest label"""
    ids, counts = np.unique(lab[lab > 0], return_counts=True)          # ids ascend, argmax takes the first maximum
    if len(ids) == 0:
        return np.zeros(lab.shape, np.uint8), 0, 0
    i = int(np.argmax(counts))
    return np.where(lab == ids[i], 255, 0).astype(np.uint8), int(counts[i]), len(ids)


def clean(src, thr=0, k=5, connectivity=8):
    """one frame [H,W] uint8 -> dict(masks, binary: uint8 0 / 255; labels int32; area, n_components: int)"""
    b = open_close(threshold(src, thr), k)
    lab = label(b, connectivity)
    m, area, n = largest(lab)
    return dict(masks=m, binary=np.where(b, 255, 0).astype(np.uint8), labels=lab, area=area, n_components=n)


def clean_batch(src, thr=0, k=5, connectivity=8):
    """[n,H,W] -> the same dict with a leading frame axis, frame by frame"""
    r = [clean(f, thr, k, connectivity) for f in src]
    return {key: np.stack([np.asarray(x[key]) for x in r]).astype(np.int32 if key in ("area", "n_components", "labels") else np.uint8)
            for key in ("masks", "binary", "labels", "area", "n_components")}


def apply(images, masks):
    """images [...,3] uint8, masks [...] uint8 -> the images, 0 outside the mask"""
    return np.where(np.asarray(masks)[..., None] != 0, images, 0).astype(np.uint8)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def serpentine(H, W):
    """a one-pixel corridor that runs along every even row and drops to the next one at alternating ends: one component whose
    first pixel is (0, 0), at either connectivity"""
    a = np.zeros((H, W), np.uint8)
    a[0::2] = 255
    for i, y in enumerate(range(1, H, 2)):
        a[y, W - 1 if i % 2 == 0 else 0] = 255
    return a


def spiral(n):
    """a one-pixel square spiral on n x n, from the corner (0, 0) inwards with a one-pixel gap between the turns: one component"""
    a = np.zeros((n, n), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    a[0, 0] = 255

    def free(yy, xx):       # inside, and the cell behind it is not part of an earlier turn
        return 0 <= yy < n and 0 <= xx < n and not a[yy, xx] and not (0 <= yy + dy < n and 0 <= xx + dx < n and a[yy + dy, xx + dx])

    turns = 0
    while turns < 2:
        if free(y + dy, x + dx):
            y, x = y + dy, x + dx
            a[y, x] = 255
            turns = 0
        else:
            dy, dx = dx, -dy
            turns += 1
    return a


def checkerboard(H, W):
    yy, xx = np.mgrid[:H, :W]
    return np.where((yy + xx) % 2 == 0, 255, 0).astype(np.uint8)


def random_mask(H, W, seed, cell=6, flip=0.03):
    """seeded blobs (a coarse random grid of cell x cell squares, 60 % set) with `flip` of the pixels inverted: blobs that survive an
    open, speckles and pinholes that do not.  Foreground values are random in 1..255, so a threshold above 0 matters too"""
    g = np.random.default_rng(seed)
    coarse = g.random(((H + cell - 1) // cell, (W + cell - 1) // cell)) < 0.6
    on = np.kron(coarse, np.ones((cell, cell), bool))[:H, :W] ^ (g.random((H, W)) < flip)
    return np.where(on, g.integers(1, 256, (H, W)), 0).astype(np.uint8)


def degrade(sil, seed, n_speckles=400, n_holes=300):
    """a clean silhouette [H,W] bool -> (raw uint8 mask, the speckle pixels [H,W] bool) as a segmentation network might leave it:
    isolated one-pixel speckles away from the body, one-pixel pinholes inside it, and a detached 12 x 9 blob in a corner"""
    g = np.random.default_rng(seed)
    sil = np.asarray(sil, bool)
    H, W = sil.shape
    raw = np.where(sil, 255, 0).astype(np.uint8)
    far = ~dilate(sil, 9)
    far[:14, :14] = False                                  # where the blob goes
    speck = np.zeros_like(sil)
    ys, xs = np.nonzero(far[::3, ::3])                     # on a stride-3 lattice: no two speckles touch
    pick = g.permutation(len(ys))[:n_speckles]
    speck[ys[pick] * 3, xs[pick] * 3] = True
    raw[speck] = g.integers(1, 256, int(speck.sum())).astype(np.uint8)
    ys, xs = np.nonzero(erode(sil, 3)[::3, ::3])
    pick = g.permutation(len(ys))[:n_holes]
    raw[ys[pick] * 3, xs[pick] * 3] = 0
    raw[2:11, 1:13] = 200
    return raw, speck


def body_silhouette(H, W, device):
    """the synthetic mesh body (synthetic.make_mesh_body) in its rest pose, rasterised from the front at H x W on `device`, filling
    0.8 of the image height -> [H,W] bool (numpy)"""
    import torch
    from instantavatar_amd import raster, synthetic
    d = synthetic.make_mesh_body()
    v = d["v_template"].astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    c, e = (lo + hi) / 2, hi - lo
    dist = 3.0
    f = 0.8 * H * (dist - e[2] / 2) / e[1]
    w2c = np.eye(4)
    R = np.diag([-1.0, -1.0, 1.0])
    w2c[:3, :3], w2c[:3, 3] = R, -R @ (c - np.array([0.0, 0.0, dist]))
    K = np.array([[f, 0, (W - 1) / 2], [0, f, (H - 1) / 2], [0, 0, 1]])
    cam = raster.Camera(K, torch.as_tensor(w2c, dtype=torch.float32, device=device), H, W)
    fr = raster.rasterize(torch.as_tensor(d["v_template"], device=device), torch.as_tensor(d["f"], device=device), cam)
    return fr.mask.cpu().numpy()
