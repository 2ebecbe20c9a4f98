"""Scene composition: several rendered avatars, a ground plane that receives their shadows and a background in one frame
(csrc/ia_scene.hip, include/instantavatar_hip_scene.h; definition in DESIGN.md section 4, "scene composition").

    ground = scene.ground_under(models, seqs, cell=0.5)
    sc = scene.Scene(models, seqs, ground=ground, light=(-2.0, -4.0, 2.0), jitter=animate.fixed_jitter(1, device))
    out = sc.render(i)            # rgb [H,W,3], alpha, depth [H,W], rgba8 [H,W,4], shade [H,W], contested (device int32)

Every avatar is rendered by `AvatarModel.render_image_fast` as it is, once for the camera; with a light and a ground it is rendered a
second time from the light for its opacity, which is what no external compositing tool can get from the RGBA frames.  The layers are
then ordered by depth per pixel and composited front to back (`composite`, a thin wrapper over the three entry points; no host read).

With `receive=True` the avatars receive shadows as well, each other's and their own (`receive`, `ia_scene_receive`): the light
render's depth sum is kept next to its opacity, and every layer's pixel -- one point, at the layer's expected depth -- is looked up in
every avatar's light-view maps before the layers are composited.

With `exact=True` the pixels that two avatars share are composited a second time from every sample of every avatar in depth order
(`composite_exact`, `ia_scene_deep_composite`; the samples are recorded by `dense_routes.render_test_deep`, a second, host-driven
pass over those pixels), which is exact where bodies intertwine along a ray; the result gains `overlap` and `interleaved`.

Two limits, both stated in the header: a layer is a whole avatar, so without `exact` the order is exact only where the avatars do not
interleave along a ray (`contested` counts the pixels where they may; the light views keep this limit with `exact` too); and
shadows are a multiplier on colours that already carry the lighting of the capture, from one point light, and none falls onto the
background (without `receive` only the ground receives any).  The scene renders eagerly: captured graphs, frames in flight and
multi-rank sharding are the single-avatar drivers' and are not used here.

Colours are in the model's channel order (the (B, G, R) order of the training images, see `drivers.animate.write_frames`)."""
import numpy as np
import torch

from . import _lib

MAX_LAYERS = 8      # IA_SCENE_MAX_LAYERS


class Ground:
    """The plane normal . x = offset; `normal` has unit length and points to the side objects stand on (in the drivers' camera +y
    points down, so a floor has normal (0, -1, 0)).  color / color2: the two colours of a checker of edge `cell` metres (cell = 0 or
    color2 = None: plain `color`), in the model's channel order.  The plane is a disc around `centre` (None: the point of the plane
    nearest to the origin): opaque inside r0, fading linearly to nothing at r1."""

    def __init__(self, normal=(0.0, -1.0, 0.0), offset=0.0, color=(0.8, 0.8, 0.8), color2=None, cell=0.0, centre=None, r0=3.0, r1=5.0):
        n = np.asarray(normal, np.float64).reshape(3)
        n = n / np.linalg.norm(n)
        self.normal = tuple(float(v) for v in n)
        self.offset = float(offset)
        self.color = tuple(float(v) for v in color)
        self.color2 = self.color if color2 is None else tuple(float(v) for v in color2)
        self.cell = 0.0 if color2 is None else float(cell)
        c = n * self.offset if centre is None else np.asarray(centre, np.float64).reshape(3)
        self.centre = tuple(float(v) for v in c)
        self.r0, self.r1 = float(r0), float(r1)
        if not 0 <= self.r0 <= self.r1:
            raise _lib.IAError("scene.Ground: the radii need 0 <= r0 <= r1, got %r, %r" % (r0, r1))


def place(seq, offset):
    """moves the avatar of an `AnimateSequence` by `offset` [3] metres: added to `transl` after the sequence has centred it"""
    seq.transl = seq.transl + torch.as_tensor(np.asarray(offset, np.float32).reshape(1, 3), device=seq.transl.device)
    return seq


@torch.no_grad()
def ground_under(models, seqs, **ground_options):
    """A floor (normal (0, -1, 0): +y points down in the drivers' camera) through the lowest body-model vertex over all frames of all
    avatars, i.e. at the largest y of `SMPL.forward`'s vertices, centred under the mean root translation.  models: one model or one
    per sequence.  One host read (four floats)."""
    if not isinstance(models, (list, tuple)):
        models = [models] * len(seqs)
    lows, roots = [], []
    for model, seq in zip(models, seqs):
        body = model.deformer.body_model
        n = len(seq)
        for f0 in range(0, n, 64):
            th = seq.thetas[f0:f0 + 64]
            out = body(betas=seq.betas.expand(th.shape[0], -1), body_pose=th[:, 3:], global_orient=th[:, :3], transl=seq.transl[f0:f0 + 64])
            lows.append(out.vertices[..., 1].max().reshape(1))
        roots.append(seq.transl.mean(0))
    y, cx, _, cz = torch.cat([torch.cat(lows).max().reshape(1), torch.stack(roots).mean(0)]).cpu().tolist()
    opts = dict(ground_options)
    opts.setdefault("centre", (cx, y, cz))
    return Ground(normal=(0.0, -1.0, 0.0), offset=-y, **opts)


def light_camera(light_pos, target, extent=2.4, size=256, device="cuda", near=0.05):
    """The `raster.Camera` of a point light at `light_pos` that looks at `target` (an avatar's root translation in that frame), built
    on the host in fp64: z = (target - light) / |target - light|; the image's down direction is world +y (the drivers' down) unless z
    is within 8 degrees of it (|z_y| > 0.99), then world +z; x = down x z normalised, y = z x x; w2c = [x; y; z | -R light].  The
    focal length size |target - light| / extent makes `extent` metres at the target's distance fill the `size`^2 map; the
    principal point is the map's centre (size - 1) / 2."""
    from .raster import Camera
    light, target = np.asarray(light_pos, np.float64).reshape(3), np.asarray(target, np.float64).reshape(3)
    z = target - light
    dist = float(np.linalg.norm(z))
    if not dist > 0:
        raise _lib.IAError("scene.light_camera: the light is at its target")
    z = z / dist
    down = np.array([0.0, 1.0, 0.0]) if abs(z[1]) <= 0.99 else np.array([0.0, 0.0, 1.0])
    x = np.cross(down, z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    w2c = np.eye(4)
    w2c[:3, :3] = np.stack([x, y, z])
    w2c[:3, 3] = -w2c[:3, :3] @ light
    f = size * dist / float(extent)
    K = np.array([[f, 0.0, (size - 1) / 2.0], [0.0, f, (size - 1) / 2.0], [0.0, 0.0, 1.0]])
    cam = Camera(K, torch.as_tensor(w2c, dtype=torch.float32, device=device), size, size, near=near)
    cam.w2c_host = w2c
    return cam


def light_rays(cam):
    """(rays_o, rays_d) [S*S,3] fp32 host arrays of a `light_camera`, exactly as `drivers.animate.make_rays` makes them from its K and
    c2w, and its projection K [R | t] [3,4] fp32 (what `ia_scene_shadow` takes)"""
    from .drivers.animate import make_rays
    w2c = cam.w2c_host
    c2w = np.linalg.inv(w2c)
    o, d = make_rays(cam.K, c2w, cam.H, cam.W)
    return o, d, (cam.K @ w2c[:3, :4]).astype(np.float32)


def _projections(cams, dev):
    """(proj [K,3,4] fp32 on the device, near) of K `light_camera`s or of a [K,3,4] tensor of projections (near = 0.05 then)"""
    if torch.is_tensor(cams):
        return cams.detach().float().reshape(-1, 3, 4).contiguous(), 0.05
    return torch.as_tensor(np.stack([light_rays_projection(cm) for cm in cams]), device=dev), min(cm.near for cm in cams)


def _receive(c, a, d, o, dr, maps_a, maps_d, cams, light, normals=None, radius=1, strength=0.6, bias_other=0.02, bias_self=0.05,
             cos0=0.0, cos1=0.25):
    """`receive` on the stacked layers c [K,R,3], a, d [K,R] and rays o, dr [R,3] -> (c_out [K,R,3], shade [K,R])"""
    K, R = int(a.shape[0]), int(a.shape[1])
    dev = a.device
    f = lambda t: t.detach().float()
    _lib.require_cuda(o, dr, maps_a, maps_d)
    if o.shape[0] != R or dr.shape[0] != R:
        raise _lib.IAError("scene.receive: %d rays for layers of %d pixels" % (o.shape[0], R))
    maps_a, maps_d = f(maps_a).contiguous(), f(maps_d).contiguous()
    proj, near = _projections(cams, dev)
    if maps_a.dim() != 3 or maps_a.shape[1] != maps_a.shape[2] or maps_a.shape != maps_d.shape or maps_a.shape[0] != K \
            or proj.shape[0] != K:
        raise _lib.IAError("scene.receive: light-view maps %s / %s and %d light cameras for %d layers"
                           % (tuple(maps_a.shape), tuple(maps_d.shape), proj.shape[0], K))
    nrm = None
    if normals is not None:
        nrm = (torch.stack([f(n).reshape(R, 3) for n in normals]) if isinstance(normals, (list, tuple)) else f(normals).reshape(K, R, 3)).contiguous()
        _lib.require_cuda(nrm)
    lx, ly, lz = (float(v) for v in np.asarray(light, np.float64).reshape(3))
    c_out, shade = torch.empty((K, R, 3), device=dev), torch.empty((K, R), device=dev)
    _lib.call("ia_scene_receive", o, dr, R, c, a, d, nrm, maps_a, maps_d, proj, K, int(maps_a.shape[1]), lx, ly, lz, int(radius),
              float(strength), near, float(bias_other), float(bias_self), float(cos0), float(cos1), c_out, shade)
    return c_out, shade


def _stack(layers, who):
    """the layers of `composite` / `receive` -> (c [K,R,3], a [K,R], d [K,R], the pixels' shape)"""
    K = len(layers)
    if not 1 <= K <= MAX_LAYERS:
        raise _lib.IAError("scene.%s: %d layers, 1 .. %d can be composited" % (who, K, MAX_LAYERS))
    shape = tuple(layers[0][1].shape)
    R = int(layers[0][1].numel())
    for rgb, alpha, depth in layers:
        _lib.require_cuda(rgb, alpha, depth)
        if alpha.numel() != R or depth.numel() != R or rgb.numel() != 3 * R:
            raise _lib.IAError("scene.%s: the layers do not cover the same pixels" % who)
    f = lambda t: t.detach().float()
    c = torch.stack([f(l[0]).reshape(R, 3) for l in layers]).contiguous()
    a = torch.stack([f(l[1]).reshape(R) for l in layers]).contiguous()
    d = torch.stack([f(l[2]).reshape(R) for l in layers]).contiguous()
    return c, a, d, shape


@torch.no_grad()
def receive(layers, rays_o, rays_d, maps_a, maps_d, cams, light, normals=None, radius=1, strength=0.6, bias_other=0.02, bias_self=0.05,
            cos0=0.0, cos1=0.25):
    """The layers of `composite` shaded by the shadows the avatars cast on each other and on themselves (`ia_scene_receive`; the
    definition is in the header).  maps_a, maps_d [K,S,S]: avatar k from the light, its opacity and its depth SUM
    (`Scene.light_view_maps`); cams: the K `light_camera`s or a [K,3,4] tensor of projections, as `shadows[1]` of `composite`; light:
    the point light [3] in the rays' frame; normals: None, or per layer (a list, or one [K,..,3] tensor) the surface normals of
    `render_image_fast(normals=True)` -- a layer whose surface faces away from the light is in its own attached shadow: the shade
    falls from 1 to 1 - strength as the cosine between normal and light direction falls from cos1 to cos0.  radius: the PCF radius
    0 .. 3 of nearest taps; bias_other / bias_self: metres by which a caster must lie nearer to the light than the receiver to
    shadow it, for another avatar and for the receiver's own.
    The bias and cosine defaults are this project's choices, not measurements: 5 cm of self-bias is roughly the thickness the
    volumetric surface is smeared over along a light ray, which nobody has measured (tools/time_scene_receive.py prints the share of
    lit pixels that shadow themselves at three biases, the evidence to look at).
    -> (shaded layers: a list of (rgb * shade, alpha, depth) shaped like the input, shade [K,..]).  One launch, no host read."""
    c, a, d, shape = _stack(layers, "receive")
    o, dr = rays_o.detach().float().reshape(-1, 3).contiguous(), rays_d.detach().float().reshape(-1, 3).contiguous()
    c_out, shade = _receive(c, a, d, o, dr, maps_a, maps_d, cams, light, normals, radius, strength, bias_other, bias_self, cos0, cos1)
    shaded = [(c_out[k].reshape(layers[k][0].shape), layers[k][1], layers[k][2]) for k in range(len(layers))]
    return shaded, shade.reshape(len(layers), *shape)


@torch.no_grad()
def composite(layers, rays_o, rays_d, ground=None, shadows=None, background=None, contact=0.3, receive=None, rows=None):
    """layers: a list of 1 .. 8 (rgb [..,3], alpha [..], depth [..]) of `render_image_fast` with a zero `bg_color` in the batch --
    premultiplied colour, opacity, depth SUM -- all over the same rays rays_o, rays_d [..,3].  ground: a `Ground`; shadows: (maps
    [K,S,S] light-view opacity, cameras: K `light_camera`s or a [K,3,4] tensor of projections, PCF radius, strength), used with a
    ground only; background: None, a colour of three numbers, a [3] tensor or an image [..,3] over the same pixels.
    receive: None, or a dict of the arguments of `receive` after the rays (maps_a, maps_d, cams, light and the options): the layers
    are shaded first, then composited; None leaves every byte and every key of the result as it is without it.
    -> dict(rgb, alpha, depth, rgba8, shade, contested) shaped like the layers; `shade` is None without a ground, `contested` a
    device int32 scalar; with `receive` also layer_shade [K,..].  Four launches at most, a pack and a zero-fill; no host read.
    rows: None, or a dict that receives the flat rows the result was made from -- c [K,R,3] (unshaded), a, d [K,R], factor [K,R] |
    None (the layers' shade), ground (t_g, a_g, c_g, shade) | None, bg, bg_const: what `composite_exact` gathers the active pixels
    from; the result does not depend on it."""
    c, a, d, shape = _stack(layers, "composite")
    c_in, layer_shade = c, None
    K, R = int(a.shape[0]), int(a.shape[1])
    dev = a.device
    f = lambda t: t.detach().float()
    if ground is not None or receive is not None:
        o, dr = f(rays_o).reshape(-1, 3).contiguous(), f(rays_d).reshape(-1, 3).contiguous()
    if receive is not None:
        c, layer_shade = _receive(c, a, d, o, dr, **receive)
    t_g = a_g = c_g = shade = None
    if ground is not None:
        _lib.require_cuda(o, dr)
        if o.shape[0] != R or dr.shape[0] != R:
            raise _lib.IAError("scene.composite: %d rays for layers of %d pixels" % (o.shape[0], R))
        t_g, a_g, c_g, P = torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty((R, 3), device=dev), torch.empty((R, 3), device=dev)
        _lib.call("ia_scene_ground", o, dr, R, *ground.normal, ground.offset, *ground.color, *ground.color2, ground.cell, *ground.centre,
                  ground.r0, ground.r1, t_g, a_g, c_g, P)
        if shadows is not None:
            maps, cams, radius, strength = shadows
            maps = f(maps).contiguous()
            proj, near = _projections(cams, dev)
            if maps.dim() != 3 or maps.shape[1] != maps.shape[2] or maps.shape[0] != proj.shape[0]:
                raise _lib.IAError("scene.composite: %s opacity maps for %d light cameras" % (tuple(maps.shape), proj.shape[0]))
            shade = torch.empty(R, device=dev)
            _lib.call("ia_scene_shadow", P, a_g, R, maps, proj, int(maps.shape[0]), int(maps.shape[1]), int(radius), float(strength), near, shade)
        else:
            shade = torch.ones(R, device=dev)
    bg, bg_const = None, 0
    if background is not None:
        bg = background if torch.is_tensor(background) else torch.as_tensor(np.asarray(background, np.float32), device=dev)
        bg = f(bg).contiguous()
        _lib.require_cuda(bg)
        if bg.numel() == 3:
            bg_const = 1
        elif bg.numel() != 3 * R:
            raise _lib.IAError("scene.composite: a background of %d values for %d pixels" % (bg.numel(), R))
    rgb, alpha, depth = torch.empty((R, 3), device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev)
    contested = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call("ia_scene_zero", contested, 1)
    _lib.call("ia_scene_composite", c, a, d, K, R, t_g, a_g, c_g, shade, bg, bg_const, float(contact), rgb, alpha, depth, contested)
    rgba8 = torch.empty((R, 4), dtype=torch.uint8, device=dev)
    _lib.call("ia_pack_rgba8", rgb, alpha, R, rgba8)
    out = dict(rgb=rgb.reshape(*shape, 3), alpha=alpha.reshape(shape), depth=depth.reshape(shape), rgba8=rgba8.reshape(*shape, 4),
               shade=None if shade is None else shade.reshape(shape), contested=contested.reshape(()))
    if receive is not None:
        out["layer_shade"] = layer_shade.reshape(K, *shape)
    if rows is not None:
        rows.update(c=c_in, a=a, d=d, factor=layer_shade, ground=None if t_g is None else (t_g, a_g, c_g, shade), bg=bg, bg_const=bg_const)
    return out


def _takes_part(c, a, d):
    """[K,R] bool: the layers that take part in step 3 of the composite (a > 0, c, a, d finite)"""
    return (a > 0) & torch.isfinite(a) & torch.isfinite(d) & torch.isfinite(c).all(-1)


def active_pixels(rows, exact_ground=False):
    """(active [n] int64 flat pixel indices, takes [K,R] bool) of the `rows` of `composite`: the pixels where at least two layers take
    part, with `exact_ground` also those where one layer and the ground do.  One host read (the size of the set)."""
    takes = _takes_part(rows["c"], rows["a"], rows["d"])
    count = takes.sum(0)
    active = count >= 2
    if exact_ground and rows["ground"] is not None:
        t_g, a_g, c_g, sh = rows["ground"]
        okg = (a_g > 0) & torch.isfinite(a_g) & torch.isfinite(t_g) & torch.isfinite(sh) & torch.isfinite(c_g).all(-1)
        active = active | ((count >= 1) & okg)
    return torch.nonzero(active).reshape(-1), takes


def deep_buffers(K, S, n, device, budget=8 << 30):
    """the zero-filled sample lists of `ia_scene_deep_composite`: dict(z, delta, sigma [K,S,n], rgb [K,S,n,3]), 24 K n S bytes"""
    need = 24 * int(K) * int(n) * int(S)
    if need > int(budget):
        raise _lib.IAError("scene: the sample lists of %d active pixels (%d layers x %d slots) take %d bytes, more than deep_budget = %d"
                           % (n, K, S, need, int(budget)))
    z = lambda *shape: torch.zeros(shape, device=device)
    return dict(z=z(K, S, n), delta=z(K, S, n), sigma=z(K, S, n), rgb=z(K, S, n, 3))


@torch.no_grad()
def composite_exact(layered, deep, active, rows, thresh=0.01):
    """The layered result of `composite` with its active pixels recomputed from every SAMPLE of every avatar (step 5 of DESIGN.md
    section 4, "scene composition"; `ia_scene_deep_composite`, the definition is in its header): the K sample lists of a pixel --
    `deep`: dict(z, delta, sigma [K,S,n], rgb [K,S,n,3]) over the n pixels `active` (flat int64 indices), as
    `dense_routes.render_test_deep` records them -- are merged by depth and composited with the ground, the shade the layers
    receive (`layer_shade` of the pixel as a colour factor) and the background of `rows` (as `composite(..., rows=...)` fills them).
    -> a new dict: the keys of `layered`, rgb / alpha / depth of the active pixels replaced and rgba8 repacked, plus `overlap` (the
    number of active pixels) and `interleaved` (the number of them where two avatars' composited samples really interleave), both
    device int32.  Every other pixel keeps its bytes.  One gather per row kind, one launch, a scatter and a pack."""
    K, S, n = (int(v) for v in deep["z"].shape)
    dev = deep["z"].device
    shape = tuple(layered["alpha"].shape)
    R = int(layered["alpha"].numel())
    if active.numel() != n or rows["a"].shape != (K, R):
        raise _lib.IAError("scene.composite_exact: sample lists of %d layers x %d pixels for %d active pixels of %d layers" % (K, n, active.numel(), rows["a"].shape[0]))
    factor = None if rows["factor"] is None else rows["factor"][:, active].contiguous()
    g = (None,) * 4 if rows["ground"] is None else tuple(x[active].contiguous() for x in rows["ground"])
    bg = rows["bg"]
    if bg is not None and not rows["bg_const"]:
        bg = bg.reshape(R, 3)[active].contiguous()
    rgb_a, alpha_a, depth_a = torch.empty((n, 3), device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
    interleaved = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call("ia_scene_zero", interleaved, 1)
    _lib.call("ia_scene_deep_composite", deep["z"], deep["delta"], deep["sigma"], deep["rgb"], K, S, n, factor, *g, bg, int(rows["bg_const"]),
              float(thresh), rgb_a, alpha_a, depth_a, interleaved)
    rgb, alpha, depth = layered["rgb"].reshape(R, 3).clone(), layered["alpha"].reshape(R).clone(), layered["depth"].reshape(R).clone()
    rgb[active], alpha[active], depth[active] = rgb_a, alpha_a, depth_a
    rgba8 = torch.empty((R, 4), dtype=torch.uint8, device=dev)
    _lib.call("ia_pack_rgba8", rgb, alpha, R, rgba8)
    out = dict(layered)
    out.update(rgb=rgb.reshape(*shape, 3), alpha=alpha.reshape(shape), depth=depth.reshape(shape), rgba8=rgba8.reshape(*shape, 4),
               overlap=torch.full((), n, dtype=torch.int32, device=dev), interleaved=interleaved.reshape(()))
    return out


def light_rays_projection(cam):
    """K [R | t] [3,4] fp32 of a camera: from the host copy a `light_camera` keeps, else from the device w2c (a host read)"""
    w2c = getattr(cam, "w2c_host", None)
    if w2c is None:
        w2c = cam.w2c.double().cpu().numpy()
    return (cam.K @ w2c[:3, :4]).astype(np.float32)


class Scene:
    """models, seqs: one `AvatarModel` and one `drivers.animate.AnimateSequence` per avatar (1 .. 8; the same model object may
    appear twice), all sequences with the camera of the first -- every avatar shares its rays.  Avatars are placed with `place`.
    ground: a `Ground`; light: the position [3] of a point light (shadows need both); shadow_size: the edge of the light-view
    opacity maps, `extent` metres wide around every avatar's root; shadow_radius / shadow_strength: PCF radius 0 .. 3 and the
    darkness of a full shadow; background: as `composite`; jitter: one occupancy-probe jitter for every render
    (`drivers.animate.fixed_jitter`; without it the occupancy probes, and with them the bytes, are random); phases: per avatar,
    frame i of the scene shows frame (i + phase) modulo the length of its sequence.
    receive: the avatars receive shadows too, each other's and their own (`receive`); needs a light, not a ground; the result of
    `render` gains `layer_shade` [K,H,W].  receive_normals: the camera renders are taken with normals=True and a surface that
    faces away from the light is in its own attached shadow (where the deformer has a normal pass: with an `SMPLDeformer` the
    term is left out); bias_other / bias_self: see `receive` -- the defaults are this project's choices, not measurements.
    Without `receive` every byte of the result is what it is without these options.
    exact: the pixels where at least two avatars take part (exact_ground: also one avatar and the ground) are recomposited from the
    avatars' samples in depth order (`composite_exact`); the result gains `overlap` and `interleaved` (device int32: the pixels
    recomposited, and those of them where the avatars' composited samples really interleave).  deep_budget: the bytes the sample
    lists may take (24 K n S for n such pixels), beyond which `render` raises; chunk: rays per call of the recording pass (it bounds
    the transient blocks only).  Every avatar needs the same MAX_SAMPLES.  Without `exact` no byte and no key changes.

    `render(i)`: per avatar one `render_image_fast` for the camera, with a zero `bg_color` so that the colour is premultiplied;
    when `lit` (a light, and a ground or `receive`) one more render from the light through `_render`, which reuses the deformer
    and the test occupancy grid the first render prepared for the frame (both depend on the pose alone, not on the rays) and of
    which the opacity and the depth sum at shadow_size^2 are kept; then `composite`.  `contested_total` (device int64) adds up the
    contested pixels over the calls."""

    def __init__(self, models, seqs, ground=None, light=None, shadow_size=256, background=None, jitter=None, shadow_radius=1,
                 shadow_strength=0.6, extent=2.4, contact=0.3, phases=None, receive=False, receive_normals=True, bias_other=0.02,
                 bias_self=0.05, exact=False, exact_ground=False, deep_budget=8 << 30, chunk=4096):
        if not isinstance(models, (list, tuple)):
            models = [models] * len(seqs)
        if len(models) != len(seqs) or not 1 <= len(seqs) <= MAX_LAYERS:
            raise _lib.IAError("scene.Scene: %d models for %d sequences; 1 .. %d avatars" % (len(models), len(seqs), MAX_LAYERS))
        first = seqs[0]
        for s in seqs:
            if (s.H, s.W) != (first.H, first.W) or not np.array_equal(s.K, first.K):
                raise _lib.IAError("scene.Scene: the sequences do not share one camera")
        self.models, self.seqs = list(models), list(seqs)
        self.ground, self.background, self.jitter = ground, background, jitter
        self.light = None if light is None else np.asarray(light, np.float64).reshape(3)
        self.receive, self.bias_other, self.bias_self = bool(receive), float(bias_other), float(bias_self)
        if self.receive and self.light is None:
            raise _lib.IAError("scene.Scene: receive=True needs a light")
        # the facing term needs a normal pass: the SMPL deformer declares `surface_normals` only to say that it has none
        self._normals = [self.receive and bool(receive_normals) and hasattr(m.deformer, "surface_normals")
                         and type(m.deformer).__name__ != "SMPLDeformer" for m in models]
        self.shadow_size, self.shadow_radius, self.shadow_strength = int(shadow_size), int(shadow_radius), float(shadow_strength)
        self.extent, self.contact = float(extent), float(contact)
        self.phases = [0] * len(seqs) if phases is None else [int(p) for p in phases]
        self.exact, self.exact_ground, self.deep_budget, self.chunk = bool(exact), bool(exact_ground), int(deep_budget), max(int(chunk), 1)
        self.H, self.W = first.H, first.W
        self.device = first.rays_o.device
        self._zero_bg = torch.zeros((1, self.H * self.W, 3), device=self.device)
        # the light cameras are built on the host: the root translations are read once, here
        self._transl_host = [s.transl.double().cpu().numpy() for s in seqs] if self.lit else None
        self.contested_total = torch.zeros((), dtype=torch.int64, device=self.device)

    @property
    def shadows(self):
        return self.light is not None and self.ground is not None

    @property
    def lit(self):
        """whether the light views are rendered"""
        return self.light is not None and (self.ground is not None or self.receive)

    def __len__(self):
        return max(len(s) for s in self.seqs)

    @torch.no_grad()
    def light_view(self, k, idx, batch):
        """the opacity [S,S] of avatar k from the light and the light's camera; the frame must be prepared (right behind the
        avatar's `render_image_fast`)"""
        alpha, _, cam = self.light_view_maps(k, idx, batch)
        return alpha, cam

    @torch.no_grad()
    def light_view_maps(self, k, idx, batch):
        """(opacity [S,S], depth SUM [S,S] in metres from the light, not divided by the opacity, the light's camera) of avatar k
        from the light; the frame must be prepared (right behind the avatar's `render_image_fast`)"""
        S = self.shadow_size
        cam = light_camera(self.light, self._transl_host[k][idx], self.extent, S, device=self.device)
        o, d, _ = light_rays(cam)
        t = lambda x: torch.as_tensor(x, device=self.device)[None]
        lb = {key: batch[key] for key in ("betas", "global_orient", "body_pose", "transl")}
        ones = torch.ones((1, S * S), device=self.device)
        dist = float(np.linalg.norm(self._transl_host[k][idx] - self.light))
        lb.update(rays_o=t(o), rays_d=t(d), near=ones * (dist - 1), far=ones * (dist + 1))
        out, _ = self.models[k]._render(lb, eval_mode=True)
        return out["alpha_coarse"].reshape(S, S), out["depth_coarse"].reshape(S, S), cam

    @torch.no_grad()
    def render(self, i):
        size = (self.H, self.W)
        first = self.seqs[0]
        layers, maps, depths, cams, normals = [], [], [], [], []
        batches, grids = [], []
        for k, (model, seq) in enumerate(zip(self.models, self.seqs)):
            idx = (int(i) + self.phases[k]) % len(seq)
            batch = seq.batch(idx)
            batch["rays_o"], batch["rays_d"] = first.rays_o, first.rays_d
            batch["bg_color"] = self._zero_bg
            batches.append(batch)
            if self._normals[k]:
                rgb, depth, alpha, _, nrm = model.render_image_fast(batch, size, jitter=self.jitter, normals=True)
                normals.append(nrm[0])
            else:
                rgb, depth, alpha, _ = model.render_image_fast(batch, size, jitter=self.jitter)
                normals.append(None)
            layers.append((rgb[0], alpha[0], depth[0]))
            if self.exact:      # the grid this layer was rendered with: the same model may serve two avatars, and the probes may be random
                g = model.renderer.density_grid_test
                grids.append((g.occ_bits.clone(), g.aabb.clone(), g.density_field.clone()))
            if self.lit:
                m, s, cam = self.light_view_maps(k, idx, batch)
                maps.append(m)
                depths.append(s)
                cams.append(cam)
        shadows = (torch.stack(maps), cams, self.shadow_radius, self.shadow_strength) if self.shadows else None
        received = None
        if self.receive:
            if any(n is not None for n in normals):      # a layer without a normal pass gets zero normals: no facing term
                normals = [torch.zeros_like(layers[k][0]) if n is None else n for k, n in enumerate(normals)]
            else:
                normals = None
            received = dict(maps_a=torch.stack(maps), maps_d=torch.stack(depths), cams=cams, light=self.light, normals=normals,
                            radius=self.shadow_radius, strength=self.shadow_strength, bias_other=self.bias_other, bias_self=self.bias_self)
        rows = {}
        out = composite(layers, first.rays_o, first.rays_d, ground=self.ground, shadows=shadows, background=self.background,
                        contact=self.contact, receive=received, **(dict(rows=rows) if self.exact else {}))
        self.contested_total += out["contested"]
        self.last_layers = layers      # the frame's unshaded (rgb, alpha, depth) per avatar: the driver's statistics read the opacities
        if self.exact:
            out = self._exact(out, rows, batches, grids)
        return out

    @torch.no_grad()
    def _exact(self, layered, rows, batches, grids):
        """pass 2 of `render` with exact=True: the samples of every avatar on the active pixels, then `composite_exact`"""
        from . import dense_routes
        from .models.structures.utils import Rays
        zero = torch.zeros((), dtype=torch.int32, device=self.device)
        active, takes = active_pixels(rows, self.exact_ground)
        n = int(active.numel())                                    # the host read: the scene renders eagerly
        if n == 0:
            return dict(layered, overlap=zero, interleaved=zero.clone())
        K = len(self.models)
        S = max(int(m.renderer.MAX_SAMPLES) for m in self.models)
        deep = deep_buffers(K, S, n, self.device, self.deep_budget)
        for k, (model, batch) in enumerate(zip(self.models, batches)):
            if int(model.renderer.MAX_SAMPLES) != S:
                raise _lib.IAError("scene.Scene: exact=True needs one MAX_SAMPLES for every avatar, got %d and %d" % (model.renderer.MAX_SAMPLES, S))
            model.deformer.prepare_deformer(batch)
            g = model.renderer.density_grid_test
            g.occ_bits.copy_(grids[k][0])
            g.aabb, g.density_field = grids[k][1], grids[k][2]
            rays = Rays(o=batch["rays_o"], d=batch["rays_d"], near=batch["near"], far=batch["far"])
            model.deformer.transform_rays_w2s(rays)
            field = lambda x, _, model=model: model.deformer(x, model.net_coarse, True)
            cols = torch.nonzero(takes[k][active]).reshape(-1)   # a ray with a_k = 0 has no sample at or above the threshold
            mine = active[cols]
            rec = {key: v[k] for key, v in deep.items()}
            for c0 in range(0, int(mine.numel()), self.chunk):     # the chunk only bounds the transient blocks
                dense_routes.render_test_deep(model.renderer, rays, field, mine[c0:c0 + self.chunk], rec, cols=cols[c0:c0 + self.chunk])
        self.last_deep, self.last_active, self.last_rows = deep, active, rows      # what the frame was merged from (the tests read them)
        return composite_exact(layered, deep, active, rows)
