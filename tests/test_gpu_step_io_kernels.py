"""The kernels that bracket a training step, each entry called through the C ABI on plain device tensors against tests/step_io_refs.py:

  A  ia_adam_step        p, m, v, step, the fp16 copy, found_inf and the gradients after the call BIT FOR BIT against `adam_ref` (torch's CPU
                         Adam with an exact FMA) after every one of a plan's calls: 1, 3 and 8 tensors per call with mixed beta pairs (both
                         forms of the lerp), learning rates as doubles and through lr_dev, one non-finite gradient element moved over every
                         float4 slot, the tails and the last tensor, every kind of skip flag, the arithmetic edges; the refusals
  B  ia_nonzero_select   integer-exact against `nonzero_select_ref`: window shapes around the wave width and past 256 rows, masks with
                         -1, 1e-40, NaN and zeros of both signs, draws at both float32 neighbours of every rank, draws without replacement
                         that run into each other, exhaust the candidates and reach the limit of 256
  C  ia_mask_edge / ia_mask_dilate   bit for bit on fractional masks, odd and even k, k larger than the image, one row, one column
  D  ia_sample_batch     bit for bit on fractional masks: both image types, both routes, bg given and NULL
  E  ia_patch_corners, ia_edge_indices (2^24 pixels included), ia_near_far   exact
  F  ia_make_rays        rays_o equal, rays_d within one float32 ulp of the float64 restatement

Every output carries a sentinel tail and every workspace is handed exactly the bytes its *_workspace_bytes function returns, with a
sentinel tail behind them: nothing may be written there.  A refused call must leave everything untouched.  tests/test_cpu_step_io_refs.py
shows on the CPU that the references are right and which mutants these comparisons reject."""
import ctypes as C

import numpy as np
import pytest
import torch

import step_io_refs as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
TAIL = 256
_FILL = {torch.float32: float(sr.SENT_F), torch.uint8: sr.SENT_B, torch.int32: int(sr.SENT_I), torch.float16: float(sr.SENT_H)}


def _lib():
    from instantavatar_amd import _lib as L
    return L


def _dev(a):
    return torch.as_tensor(np.array(a, order="C")).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _out(n, dtype=torch.float32):
    return torch.full((n + TAIL,), _FILL[dtype], dtype=dtype, device=DEV)


def _tail_intact(t, n, what):
    tail = _np(t[n:])
    want = np.full(1, _FILL[t.dtype], tail.dtype)
    assert len(tail) >= TAIL and (tail.view(np.uint8) == np.resize(want.view(np.uint8), tail.nbytes)).all(), ("written behind the end", what)


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    u = {2: np.uint16, 4: np.uint32, 1: np.uint8}[got.dtype.itemsize]
    bad = np.nonzero(got.reshape(-1).view(u) != want.reshape(-1).view(u))[0]
    assert not len(bad), (what, "%d of %d differ" % (len(bad), got.size), bad[:5].tolist(), got.reshape(-1)[bad[:5]].tolist(), want.reshape(-1)[bad[:5]].tolist())


def _refused(code, fn, *args):
    L = _lib()
    with pytest.raises(L.IAError) as e:
        L.call(fn, *args)
    torch.cuda.synchronize()
    assert "(%d)" % code in str(e.value), str(e.value)
    return str(e.value)


# ---- A ---------------------------------------------------------------------------------------------------------------
class _AdamDevice:
    """the device side of one plan: every buffer with a sentinel tail, the workspace exactly ia_adam_workspace_bytes() (zero-filled once)"""

    def __init__(self, plan):
        L = _lib()
        self.plan = plan
        self.ws_bytes = int(L.call("ia_adam_workspace_bytes"))
        self.ws = _out(self.ws_bytes, torch.uint8)
        self.ws[:self.ws_bytes] = 0
        self.t = []
        for t in plan["tensors"]:
            n = t["numel"]
            d = dict(n=n, p=_out(n), g=_out(n), m=_out(n), v=_out(n), step=_out(1), lr_dev=_out(1) if t["lr_dev"] else None,
                     shadow=_out(n, torch.float16) if t["has_shadow"] else None)
            d["p"][:n] = _dev(t["p0"])
            d["m"][:n] = 0
            d["v"][:n] = 0
            d["step"][:1] = float(t["step0"])
            self.t.append(d)
        self.skip = _out(1)
        self.found = _out(1)

    def items(self, lrs):
        L = _lib()
        items = []
        for t, d, lr in zip(self.plan["tensors"], self.t, lrs):
            if d["lr_dev"] is not None:
                d["lr_dev"][:1] = float(lr)
            items.append(L.AdamTensor(param=d["p"].data_ptr(), grad=d["g"].data_ptr(), exp_avg=d["m"].data_ptr(), exp_avg_sq=d["v"].data_ptr(),
                                      shadow=d["shadow"].data_ptr() if d["shadow"] is not None else None, step=d["step"].data_ptr(),
                                      lr_dev=d["lr_dev"].data_ptr() if d["lr_dev"] is not None else None, lr=0.0 if d["lr_dev"] is not None else float(lr),
                                      beta1=t["beta1"], beta2=t["beta2"], eps=t["eps"], numel=d["n"]))
        return items

    def call(self, st):
        L = _lib()
        for d, g in zip(self.t, st["g"]):
            d["g"][:d["n"]] = _dev(g)
        items = self.items(st["lrs"])
        skip = None
        if st["skip_in"] is not None:
            self.skip[:1] = _dev(np.array([st["skip_in"]], F))
            skip = self.skip
        self.found[:1] = float(sr.SENT_F)
        L.call("ia_adam_step", (L.AdamTensor * len(items))(*items), len(items), skip, self.found if st["want_found"] else None, 1 if st["zero_grad"] else 0,
               self.ws, self.ws_bytes)
        torch.cuda.synchronize()

    def check(self, snap, st, what):
        for i, d in enumerate(self.t):
            n = d["n"]
            for key in ("p", "m", "v", "g"):
                _tail_intact(d[key], n, (what, i, key))
                _same_bits(_np(d[key][:n]), snap[key][i], (what, "tensor %d of %s" % (i, self.plan["numels"]), key))
            _tail_intact(d["step"], 1, (what, i, "step"))
            assert float(d["step"][0]) == snap["step"][i], (what, i, float(d["step"][0]), snap["step"][i])
            if d["shadow"] is not None:
                _tail_intact(d["shadow"], n, (what, i, "shadow"))
                _same_bits(_np(d["shadow"][:n]), snap["shadow"][i], (what, i, "shadow"))
            if d["lr_dev"] is not None:
                _tail_intact(d["lr_dev"], 1, (what, i, "lr_dev"))
        _tail_intact(self.ws, self.ws_bytes, (what, "workspace"))
        assert not _np(self.ws[:self.ws_bytes]).any(), (what, "the flag is cleared for the next step")
        _tail_intact(self.found, 1, (what, "found_inf"))
        _tail_intact(self.skip, 1, (what, "skip_in"))
        want = (1.0 if snap["found"] else 0.0) if st["want_found"] else float(sr.SENT_F)
        assert float(self.found[0]) == want, (what, float(self.found[0]), want)


@pytest.fixture(scope="module")
def adam_plans():
    return sr.adam_plans()


N_ADAM_PLANS = len(sr.adam_groupings()) + len(sr.ADAM_BAD_POSITIONS)


@pytest.mark.parametrize("i", range(N_ADAM_PLANS))
def test_adam_step_bit_for_bit(adam_plans, i):
    assert len(adam_plans) == N_ADAM_PLANS
    plan = adam_plans[i]
    ref = sr.adam_run_ref(plan)
    dev = _AdamDevice(plan)
    n_lerp_end = sum(F(1 - t["beta1"]) >= F(0.5) for t in plan["tensors"])
    for k, (st, snap) in enumerate(zip(plan["steps"], ref)):
        dev.call(st)
        dev.check(snap, st, "plan %d step %d" % (i, k))
        assert snap["found"] == st["expect_skip"]
    print("adam plan %d: numels %s, %d tensor(s) on the large-weight lerp, non-finite element at %s: %d calls bit for bit" % (i, plan["numels"], n_lerp_end, plan["bad"], len(ref)))


def test_adam_step_refusals_leave_everything_untouched(adam_plans):
    L = _lib()
    plan = sr.adam_plan((8, 5), 0)
    dev = _AdamDevice(plan)
    st = plan["steps"][0]
    for d, g in zip(dev.t, st["g"]):
        d["g"][:d["n"]] = _dev(g)
    before = [{k: _np(d[k]).copy() for k in ("p", "g", "m", "v", "step", "shadow") if d[k] is not None} for d in dev.t]
    base = dev.items(st["lrs"])

    def variant(**kw):
        items = dev.items(st["lrs"])
        for k, v in kw.items():
            setattr(items[0], k, v)
        return items

    nine = (base * 5)[:9]
    cases = [("0 tensors", base, 0, dev.ws_bytes, sr.IA_ERR_ARG), ("9 tensors", nine, 9, dev.ws_bytes, sr.IA_ERR_ARG),
             ("numel 0", variant(numel=0), 2, dev.ws_bytes, sr.IA_ERR_ARG),
             ("param + 4 bytes", variant(param=dev.t[0]["p"].data_ptr() + 4), 2, dev.ws_bytes, sr.IA_ERR_ARG),
             ("shadow + 2 bytes", variant(shadow=dev.t[0]["shadow"].data_ptr() + 2), 2, dev.ws_bytes, sr.IA_ERR_ARG),
             ("beta1 = 1", variant(beta1=1.0), 2, dev.ws_bytes, sr.IA_ERR_ARG),
             ("workspace one byte short", base, 2, dev.ws_bytes - 1, sr.IA_ERR_WORKSPACE)]
    assert dev.t[0]["shadow"] is not None
    for name, items, n, ws_bytes, code in cases:
        msg = _refused(code, "ia_adam_step", (L.AdamTensor * len(items))(*items), n, None, dev.found, 1, dev.ws, ws_bytes)
        assert "ia_adam_step" in msg, (name, msg)
        for d, b in zip(dev.t, before):
            for k, a in b.items():
                assert np.array_equal(_np(d[k]).view(np.uint8), a.view(np.uint8)), (name, k)
        assert float(dev.found[0]) == float(sr.SENT_F) and not _np(dev.ws[:dev.ws_bytes]).any(), name
    # and the same call with nothing wrong goes through
    dev.call(st)
    dev.check(sr.adam_run_ref(plan)[0], st, "after the refusals")


# ---- B ---------------------------------------------------------------------------------------------------------------
def _select(mask_dev, frame, u, without_replacement=False, with_count=True, ws_short=0, refused=False):
    """one call with exactly its workspace; (rows, cols, count or None).  refused: the call must raise and leave everything untouched"""
    L = _lib()
    H, W, y0, y1, x0, x1 = frame
    n = len(u)
    nbytes = int(L.call("ia_nonzero_select_workspace_bytes", y1 - y0, n))
    ws, rows, cols, count = _out(nbytes, torch.uint8), _out(n, torch.int32), _out(n, torch.int32), _out(1, torch.int32)
    u_dev = _dev(np.asarray(u, F)) if n else _out(1)
    try:
        L.call("ia_nonzero_select", mask_dev, H, W, y0, y1, x0, x1, u_dev, n, 1 if without_replacement else 0, rows, cols, count if with_count else None,
               ws, nbytes - ws_short)
    finally:
        torch.cuda.synchronize()
        _tail_intact(ws, 0 if refused else nbytes, "select workspace")
        _tail_intact(rows, 0 if refused else n, "out_row")
        _tail_intact(cols, 0 if refused else n, "out_col")
        _tail_intact(count, 1 if with_count and not refused else 0, "count_out")
    return _np(rows[:n]), _np(cols[:n]), (int(count[0]) if with_count else None)


@pytest.mark.parametrize("rows,cols", sr.SELECT_WINDOWS)
def test_nonzero_select_with_replacement(rows, cols):
    for fi, frame in enumerate(sr.select_frames(rows, cols)):
        win = frame[2:]
        for kind in ("mixed", "last_only", "all_zero"):
            mask = sr.select_mask(frame, kind, rows * 7 + cols + fi)
            mask_dev = _dev(mask)
            count = sr.nonzero_select_ref(mask, win, [])[2]
            assert (kind != "last_only" or count == 1) and (kind != "all_zero" or count == 0)
            draws = sr.select_draws(count, 500, rows + cols)
            calls = [draws[:n] for n in sr.SELECT_NS[:-1]] + sr.chunks(draws, 500)
            for j, u in enumerate(calls):
                want = sr.nonzero_select_ref(mask, win, u)
                got = _select(mask_dev, frame, u, with_count=j % 2 == 0)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (frame, kind, len(u), got[0][:8], want[0][:8], got[1][:8], want[1][:8])
                assert got[2] is None or got[2] == want[2] == count, (frame, kind, got[2], want[2])
            print("select %s %s: %d candidates, %d calls exact" % (frame, kind, count, len(calls)))


def test_nonzero_select_without_replacement():
    for name, frame, count, u in sr.without_replacement_cases():
        mask = sr.select_mask(frame, "count", 3, count=count)
        want = sr.nonzero_select_ref(mask, frame[2:], u, without_replacement=True)
        got = _select(_dev(mask), frame, u, without_replacement=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] == count, (name, got[0][:8], want[0][:8])
        n_valid = min(len(u), count)
        assert len(set(zip(got[0][:n_valid].tolist(), got[1][:n_valid].tolist()))) == n_valid and (got[0][n_valid:] == -1).all(), name
    # the mixed masks too (NaN and denormal candidates), a few draws
    for rows, cols in ((5, 130), (513, 2)):
        frame = sr.select_frames(rows, cols)[0]
        mask = sr.select_mask(frame, "mixed", 99)
        u = np.random.RandomState(rows).rand(16).astype(F)
        want = sr.nonzero_select_ref(mask, frame[2:], u, without_replacement=True)
        got = _select(_dev(mask), frame, u, without_replacement=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_nonzero_select_refusals():
    frame = sr.select_frames(5, 130)[0]
    H, W, y0, y1, x0, x1 = frame
    mask_dev = _dev(sr.select_mask(frame, "mixed", 1))
    L = _lib()
    with pytest.raises(L.IAError) as e:
        _select(mask_dev, frame, np.zeros(257, F), without_replacement=True, refused=True)
    assert "(%d)" % sr.IA_ERR_ARG in str(e.value) and "256" in str(e.value)
    for bad in ((H, W, y1, y1, x0, x1), (H, W, y1, y0, x0, x1), (H, W, y0, y1, x0, W + 1), (H, W, y0, H + 1, x0, x1), (H, W, -1, y1, x0, x1)):
        with pytest.raises(L.IAError) as e:
            _select(mask_dev, bad, np.zeros(4, F), refused=True)
        assert "(%d)" % sr.IA_ERR_ARG in str(e.value) and "bad window" in str(e.value), bad
    with pytest.raises(L.IAError) as e:
        _select(mask_dev, frame, np.zeros(4, F), ws_short=1, refused=True)
    assert "(%d)" % sr.IA_ERR_WORKSPACE in str(e.value)
    _select(mask_dev, frame, np.zeros(256, F), without_replacement=True)                       # 256 draws are taken


# ---- C ---------------------------------------------------------------------------------------------------------------
def _morph(entry, mask, k, ws_short=0, refused=False):
    L = _lib()
    H, W = mask.shape
    nbytes = int(L.call("ia_mask_edge_workspace_bytes", H, W))
    ws, out = _out(nbytes, torch.uint8), _out(H * W)
    try:
        L.call(entry, _dev(mask), H, W, k, out, ws, nbytes - ws_short)
    finally:
        torch.cuda.synchronize()
        _tail_intact(ws, 0 if refused else nbytes, entry + " workspace")
        _tail_intact(out, 0 if refused else H * W, entry)
    return _np(out[:H * W]).reshape(H, W)


@pytest.mark.parametrize("H,W,k", sr.MORPH_CASES)
def test_mask_edge_and_dilate_bit_for_bit(H, W, k):
    for name, m in sr.morph_masks(H, W).items():
        _same_bits(_morph("ia_mask_edge", m, k), sr.edge_band_ref(m, k), ("edge", H, W, k, name))
        _same_bits(_morph("ia_mask_dilate", m, k), sr.dilate_ref(m, k), ("dilate", H, W, k, name))


def test_mask_edge_and_dilate_refusals():
    L = _lib()
    m = sr.morph_masks(9, 7)["blobs"]
    for entry in ("ia_mask_edge", "ia_mask_dilate"):
        for k, short, code in ((0, 0, sr.IA_ERR_ARG), (-3, 0, sr.IA_ERR_ARG), (3, 1, sr.IA_ERR_WORKSPACE)):
            with pytest.raises(L.IAError) as e:
                _morph(entry, m, k, ws_short=short, refused=True)
            assert "(%d)" % code in str(e.value), (entry, k, str(e.value))


# ---- D ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    frame = sr.batch_frame()
    return frame, {k: _dev(v) for k, v in frame.items()}


def _sample_batch(dev, n, flat=None, corners=None, patch=0, n_patch=0, bg=None, use_float=False, extras=True, expect_error=False):
    L = _lib()
    room = max(n, 0)
    outs = dict(rgb=_out(3 * room), alpha=_out(room), o=_out(3 * room), d=_out(3 * room), bg=_out(3 * room), idx=_out(room, torch.int32))
    rows, cols = (None, None) if corners is None else (_dev(corners[0]), _dev(corners[1]))
    args = (None if use_float else dev["u8"], dev["img_f"] if use_float else None, dev["mask"], dev["rays_o"], dev["rays_d"], sr.BATCH_H, sr.BATCH_W,
            None if flat is None else _dev(flat), rows, cols, n_patch, patch, n, None if bg is None else _dev(bg), outs["rgb"], outs["alpha"], outs["o"], outs["d"],
            outs["bg"] if extras else None, outs["idx"] if extras else None)
    if expect_error:
        msg = _refused(sr.IA_ERR_ARG, "ia_sample_batch", *args)
        for k, t in outs.items():
            _tail_intact(t, 0, k + " after a refusal")
        return msg
    L.call("ia_sample_batch", *args)
    torch.cuda.synchronize()
    for k, t in outs.items():
        per = 3 if k in ("rgb", "o", "d", "bg") else 1
        _tail_intact(t, per * n if (extras or k not in ("bg", "idx")) else 0, k)
    return tuple(_np(outs[k][:(3 if k in ("rgb", "o", "d", "bg") else 1) * n]) for k in ("rgb", "alpha", "o", "d", "bg", "idx"))


def _check_batch(got, want, extras, what):
    for j, name in enumerate(("rgb", "alpha", "rays_o", "rays_d", "bg_out", "idx_out")):
        if extras or j < 4:
            _same_bits(got[j].reshape(want[j].shape), want[j], (what, name))


@pytest.mark.parametrize("use_float", (False, True))
def test_sample_batch_bit_for_bit(batch, use_float):
    frame, dev = batch
    rs = np.random.RandomState(3)
    for n in sr.BATCH_FLAT_NS:
        idx = sr.batch_flat_indices(n)
        for bg in (rs.rand(n, 3).astype(F), None):
            for extras in (True, False):
                got = _sample_batch(dev, n, flat=idx, bg=bg, use_float=use_float, extras=extras)
                _check_batch(got, sr.sample_batch_ref(frame, sr.BATCH_W, flat_idx=idx, bg=bg, use_float_image=use_float), extras, ("flat", n, bg is None))
    for patch, n_patch in sr.BATCH_PATCHES:
        corners = sr.batch_corners(patch, n_patch)
        n = n_patch * patch * patch
        for bg in (rs.rand(n, 3).astype(F), None):
            got = _sample_batch(dev, n, corners=corners, patch=patch, n_patch=n_patch, bg=bg, use_float=use_float, extras=bg is not None)
            _check_batch(got, sr.sample_batch_ref(frame, sr.BATCH_W, corners=corners, patch=patch, bg=bg, use_float_image=use_float), bg is not None,
                         ("patch", patch, n_patch, bg is None))


def test_sample_batch_empty_and_refused(batch):
    frame, dev = batch
    # n = 0 writes nothing, whatever else is passed
    _sample_batch(dev, 0, flat=np.zeros(1, np.int32), bg=None)
    corners = sr.batch_corners(3, 4)
    msg = _sample_batch(dev, 35, corners=corners, patch=3, n_patch=4, expect_error=True)              # 35 != 4 * 9
    assert "n_patch" in msg
    _sample_batch(dev, 36, corners=corners, patch=0, n_patch=4, expect_error=True)
    _sample_batch(dev, 36, expect_error=True)                                                          # neither route
    _sample_batch(dev, -1, flat=np.zeros(1, np.int32), expect_error=True)


# ---- E ---------------------------------------------------------------------------------------------------------------
def test_patch_corners_exact():
    L = _lib()
    for name, H, W, P, ratio, n, draws, rm, cm in sr.corner_cases():
        rows, cols = _out(n, torch.int32), _out(n, torch.int32)
        L.call("ia_patch_corners", _dev(rm), _dev(cm), _dev(draws), n, H, W, P, float(F(ratio)), rows, cols)
        torch.cuda.synchronize()
        _tail_intact(rows, n, name)
        _tail_intact(cols, n, name)
        want = sr.patch_corners_ref(rm, cm, draws, n, H, W, P, ratio)
        assert np.array_equal(_np(rows[:n]), want[0]) and np.array_equal(_np(cols[:n]), want[1]), (name, _np(rows[:n])[:8], want[0][:8])
    one = _out(1, torch.int32)
    _refused(sr.IA_ERR_ARG, "ia_patch_corners", one, one, _out(3), 1, 16, 64, 16, 1.0, one, one)     # H <= patch
    _tail_intact(one, 0, "refused ia_patch_corners")


def test_edge_indices_exact_up_to_two_to_the_24_pixels():
    L = _lib()
    opt = lambda a: _dev(a) if len(a) else None
    for name, H, W, nm, ne, nr, draws, r_m, c_m, r_e, c_e in sr.edge_index_cases():
        n = nm + ne + nr
        out = _out(n, torch.int32)
        L.call("ia_edge_indices", opt(r_m), opt(c_m), opt(r_e), opt(c_e), _dev(draws), nm, ne, nr, H, W, out)
        torch.cuda.synchronize()
        _tail_intact(out, n, name)
        assert np.array_equal(_np(out[:n]), sr.edge_indices_ref(r_m, c_m, r_e, c_e, draws, nm, ne, nr, H, W)), name
    # 2^24 pixels (the largest frame the entry takes): the float32 below 1 gives the last pixel, not the one behind it.  Output only.
    draws = np.array([sr.ONE_BELOW, 0, 0.5, 1.0], F)
    out = _out(4, torch.int32)
    L.call("ia_edge_indices", None, None, None, None, _dev(draws), 0, 0, 4, 4096, 4096, out)
    torch.cuda.synchronize()
    _tail_intact(out, 4, "2^24 pixels")
    assert _np(out[:4]).tolist() == [2 ** 24 - 1, 0, 2 ** 23, 2 ** 24 - 1]
    assert _np(out[:4]).tolist() == sr.edge_indices_ref(None, None, None, None, draws, 0, 0, 4, 4096, 4096).tolist()
    msg = _refused(sr.IA_ERR_ARG, "ia_edge_indices", None, None, None, None, _dev(draws), 0, 0, 4, 4097, 4096, out)
    assert "2^24" in msg
    _tail_intact(out, 4, "refused ia_edge_indices")
    assert _np(out[:4]).tolist() == [2 ** 24 - 1, 0, 2 ** 23, 2 ** 24 - 1]


def test_near_far_exact():
    L = _lib()
    for n in sr.NEAR_FAR_NS:
        for t in sr.NEAR_FAR_TRANSL:
            near, far = _out(n), _out(n)
            L.call("ia_near_far", _dev(np.array(t, F)), n, near, far)
            torch.cuda.synchronize()
            _tail_intact(near, n, "near")
            _tail_intact(far, n, "far")
            want = sr.near_far_ref(t)
            _same_bits(_np(near[:n]), np.full(n, want[0], F), ("near", t, n))
            _same_bits(_np(far[:n]), np.full(n, want[1], F), ("far", t, n))


# ---- F ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", sr.RAY_SHAPES)
def test_make_rays_within_one_ulp_of_float64(H, W):
    L = _lib()
    K, R, t = sr.ray_camera(H, W)
    K_inv = np.linalg.inv(K)
    arr = lambda a: (C.c_double * a.size)(*np.asarray(a, np.float64).reshape(-1).tolist())
    n = H * W
    o, d = _out(3 * n), _out(3 * n)
    L.call("ia_make_rays", arr(K_inv), arr(R), arr(t), H, W, o, d)
    torch.cuda.synchronize()
    _tail_intact(o, 3 * n, "rays_o")
    _tail_intact(d, 3 * n, "rays_d")
    ro, rd = sr.make_rays_ref(K_inv, R, t, H, W)
    _same_bits(_np(o[:3 * n]).reshape(n, 3), ro.astype(F), "rays_o")
    err = np.abs(_np(d[:3 * n]).reshape(n, 3).astype(np.float64) - rd)
    print("make_rays %d x %d: max |rays_d - float64| %.3g (allowance %.3g), %d of %d differ from the rounded float64" % (
        H, W, err.max(), sr.RAY_ULP, int((_np(d[:3 * n]).reshape(n, 3) != rd.astype(F)).sum()), 3 * n))
    assert err.max() <= sr.RAY_ULP
