"""Float64 numpy references of the mesh extraction ("isosurface"; include/instantavatar_hip_mesh.h),
written from the rules, not from the generated table of csrc/ia_mt_table.h: brute-force marching tetrahedra over the
cells of a lattice, connected components with their areas, forward skinning, a PLY / OBJ reader and the helpers the mesh
tests share."""
import itertools

import numpy as np

SLOTS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
DEFAULT_BOX = (np.float32([-1.0, -1.0, -1.0]), np.float32([1.0, 1.0, 1.0]))


# ---- lattice ----------------------------------------------------------------------------------------------------------
def lattice_points32(N, lo, hi, first=0, count=None):
    """positions of lattice points first .. first + count in linear order, the fp32 formula: lo + (hi - lo) * (i / (N - 1))"""
    count = N ** 3 - first if count is None else count
    lin = np.arange(first, first + count, dtype=np.int64)
    ijk = np.stack([lin // (N * N), lin // N % N, lin % N], 1)
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    frac = (ijk.astype(np.float32) / np.float32(N - 1)).astype(np.float32)
    return (lo[None] + ((hi - lo).astype(np.float32)[None] * frac).astype(np.float32)).astype(np.float32)


def lattice_points64(N, lo, hi):
    lo, hi = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    g = np.stack(np.meshgrid(*[np.arange(N)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    return lo[None] + (hi - lo)[None] * (g / (N - 1))


def effective_scalar(sigma, N, cap):
    """the scalar the extractor classifies and interpolates: fp32, non-finite -> 0, the outermost layer -> 0 with cap"""
    s = np.asarray(sigma, np.float32).reshape(N, N, N).copy()
    s[~np.isfinite(s)] = 0
    if cap:
        s[0], s[-1], s[:, 0], s[:, -1], s[:, :, 0], s[:, :, -1] = 0, 0, 0, 0, 0, 0
    return s


# ---- marching tetrahedra ----------------------------------------------------------------------------------------------
def kuhn_tets():
    tets = []
    for a, b, _ in itertools.permutations(range(3)):
        v1 = np.zeros(3, int)
        v1[a] = 1
        v2 = v1.copy()
        v2[b] = 1
        tets.append(np.array([[0, 0, 0], v1, v2, [1, 1, 1]]))
    return tets


def tet_triangles(vs, case):
    """triangles of a tetrahedron with local vertices vs [4,3] for the 4-bit inside mask `case`: a list of triangles, each
    three (i, j) local vertex pairs, wound so that the normal at the edge midpoints points from the inside to the outside"""
    ins = [i for i in range(4) if case >> i & 1]
    outs = [i for i in range(4) if not case >> i & 1]
    if len(ins) == 1:
        tris = [[(ins[0], o) for o in outs]]
    elif len(ins) == 3:
        tris = [[(i, outs[0]) for i in ins]]
    elif len(ins) == 2:
        (a, b), (c, d) = ins, outs
        tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
    else:
        return []
    vs = np.asarray(vs, np.float64)
    direction = vs[outs].mean(0) - vs[ins].mean(0)
    out = []
    for t in tris:
        m = [(vs[i] + vs[j]) / 2 for i, j in t]
        n = np.cross(m[1] - m[0], m[2] - m[0])
        out.append(t if n @ direction > 0 else [t[0], t[2], t[1]])
    return out


def marching_tets(sigma, N, level=10.0, lo=DEFAULT_BOX[0], hi=DEFAULT_BOX[1], cap=True):
    """-> (verts [nv,3] float64, faces [nf,3] int32, face_cell [nf]) in the order the definition fixes: vertices by
    ascending owner * 7 + slot, faces by cell, tetrahedron, triangle.  sigma: the fp32 lattice, so `s > level` is decided on
    the same bits as in the kernel."""
    s = effective_scalar(sigma, N, cap)
    level32 = np.float32(level)
    inside = s > level32
    M = N - 1
    ci, cj, ck = [a.reshape(-1) for a in np.meshgrid(*[np.arange(M)] * 3, indexing="ij")]
    cell = (ci * M + cj) * M + ck
    rows = []
    for k, vs in enumerate(kuhn_tets()):
        case = np.zeros(len(cell), int)
        for v in range(4):
            case |= inside[ci + vs[v, 0], cj + vs[v, 1], ck + vs[v, 2]].astype(int) << v
        for c in range(1, 15):
            sel = np.nonzero(case == c)[0]
            if not len(sel):
                continue
            for t, tri in enumerate(tet_triangles(vs, c)):
                keys = []
                for i, j in tri:
                    i, j = min(i, j), max(i, j)
                    owner = ((ci[sel] + vs[i, 0]) * N + cj[sel] + vs[i, 1]) * N + ck[sel] + vs[i, 2]
                    keys.append(owner * 7 + SLOTS.index(tuple(vs[j] - vs[i])))
                rows.append(np.stack([cell[sel], np.full(len(sel), k), np.full(len(sel), t)] + keys, 1))
    if not rows:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int32), np.zeros(0, np.int64)
    rows = np.concatenate(rows)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    uniq = np.unique(rows[:, 3:])
    faces = np.searchsorted(uniq, rows[:, 3:]).astype(np.int32)
    owner, slot = uniq // 7, uniq % 7
    other = owner + np.array([(d[0] * N + d[1]) * N + d[2] for d in SLOTS])[slot]
    P = lattice_points64(N, lo, hi)
    sf = s.reshape(-1).astype(np.float64)
    t = (np.float64(level32) - sf[owner]) / (sf[other] - sf[owner])
    verts = P[owner] + t[:, None] * (P[other] - P[owner])
    return verts, faces, rows[:, 0]


# ---- mesh helpers -----------------------------------------------------------------------------------------------------
def canonical_faces(faces):
    """every face rotated so that its smallest index comes first (the winding is kept)"""
    f = np.asarray(faces).reshape(-1, 3)
    r = f.argmin(1)
    idx = (r[:, None] + np.arange(3)[None]) % 3
    return np.take_along_axis(f, idx, 1)


def directed_edge_counts(faces):
    """{(a, b): uses} over the directed edges of the faces"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key, cnt = np.unique(e[:, 0] * (1 << 32) + e[:, 1], return_counts=True)
    return {(int(k >> 32), int(k & 0xffffffff)): int(c) for k, c in zip(key, cnt)}


def is_closed_oriented(faces):
    """every directed edge used exactly once and its reverse exactly once"""
    d = directed_edge_counts(faces)
    return all(c == 1 and d.get((b, a), 0) == 1 for (a, b), c in d.items())


def euler_characteristic(nv, faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    return nv - len(np.unique(e[:, 0] * (1 << 32) + e[:, 1])) + len(f)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ni,ni->n", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6)


def face_areas(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)


def components(verts, faces):
    """-> (label [nv]: the smallest vertex index of the vertex's component, {label: surface area}); faces connect through
    shared vertices"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    label = np.arange(len(verts))
    while True:
        m = label[f].min(1)
        new = label.copy()
        for c in range(3):
            np.minimum.at(new, f[:, c], m)
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    area = {}
    fa = face_areas(verts, f)
    for l in np.unique(label[f[:, 0]]) if len(f) else []:
        area[int(l)] = float(fa[label[f[:, 0]] == l].sum())
    return label, area


def largest_component(verts, faces):
    """-> (verts_out, faces_out, vert_src): the component with the largest area (ties: the smallest root vertex), the kept
    vertices and faces in their old order"""
    label, area = components(verts, faces)
    best = min(area, key=lambda l: (-area[l], l))
    keep = label == best
    src = np.nonzero(keep)[0]
    new = np.full(len(verts), -1, np.int64)
    new[src] = np.arange(len(src))
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.asarray(verts)[src], new[f[keep[f[:, 0]]]].astype(np.int32), src.astype(np.int32)


# ---- forward skinning -------------------------------------------------------------------------------------------------
def forward_skin_ref(xc, voxel_J, grid, s2w):
    """x_d = s2w (J(x_c) [x_c; 1]) in float64, J the trilinear blend of voxel_J [D,H,W,12] (corners outside the grid with
    weight 0; the source index is formed in fp32 as the kernel forms it, which decides the cell).  -> (x_d [n,3], mag [n,3]:
    per output the sum of the absolute values of the terms it is made of, the scale of its rounding error)"""
    xc = np.asarray(xc, np.float32)
    D, H, W = grid["D"], grid["H"], grid["W"]
    off, scl = np.asarray(grid["offset"], np.float32), np.asarray(grid["scale"], np.float32)
    gn = (scl[None] * (xc + off[None]).astype(np.float32)).astype(np.float32)
    sizes = (W, H, D)
    with np.errstate(all="ignore"):
        ix = [(((gn[:, a] + np.float32(1)) / np.float32(2)).astype(np.float32) * np.float32(sizes[a] - 1)).astype(np.float32) for a in range(3)]
    ix = [np.where(np.abs(v) <= 2147483648.0, v, np.float32(-100.0)).astype(np.float32) for v in ix]
    i0 = [np.floor(v).astype(np.int64) for v in ix]
    fr = [v.astype(np.float64) - f for v, f in zip(ix, i0)]
    vJ = np.asarray(voxel_J, np.float64).reshape(D, H, W, 3, 4)
    n = len(xc)
    J, Ja = np.zeros((n, 3, 4)), np.zeros((n, 3, 4))
    for c in range(8):
        cx, cy, cz = i0[0] + (c & 1), i0[1] + ((c >> 1) & 1), i0[2] + ((c >> 2) & 1)
        wx = fr[0] if c & 1 else 1 - fr[0]
        wy = fr[1] if c & 2 else 1 - fr[1]
        wz = fr[2] if c & 4 else 1 - fr[2]
        ok = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H) & (cz >= 0) & (cz < D)
        w = np.where(ok, wx * wy * wz, 0.0)
        rec = vJ[np.clip(cz, 0, D - 1), np.clip(cy, 0, H - 1), np.clip(cx, 0, W - 1)]
        J += w[:, None, None] * rec
        Ja += w[:, None, None] * np.abs(rec)
    x1 = np.concatenate([xc.astype(np.float64), np.ones((n, 1))], 1)
    y = np.einsum("nij,nj->ni", J, x1)
    ya = np.einsum("nij,nj->ni", Ja, np.abs(x1))
    S = np.asarray(s2w, np.float64).reshape(4, 4)
    xd = y @ S[:3, :3].T + S[:3, 3]
    mag = ya @ np.abs(S[:3, :3]).T + np.abs(S[:3, 3])
    return xd, mag


# ---- files ------------------------------------------------------------------------------------------------------------
PLY_TYPES = {"float": "<f4", "uchar": "u1", "int": "<i4", "int32": "<i4", "float32": "<f4", "uint8": "u1"}


def read_ply(path):
    """binary little-endian PLY with a vertex element of scalar properties and a face element `list uchar int32 vertex_indices`
    of triangles -> dict(vertex = structured array, faces [nf,3] int32, header = text, payload_bytes = bytes behind it)"""
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    header = blob[:end].decode("ascii")
    lines = header.split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    elements, cur = [], None
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            cur = dict(name=w[1], n=int(w[2]), props=[])
            elements.append(cur)
        elif w[:1] == ["property"]:
            cur["props"].append(w[1:])
    assert [e["name"] for e in elements] == ["vertex", "face"], elements
    vdt = np.dtype([(p[1], PLY_TYPES[p[0]]) for p in elements[0]["props"]])
    nv, nf = elements[0]["n"], elements[1]["n"]
    assert elements[1]["props"] == [["list", "uchar", "int", "vertex_indices"]] or \
        elements[1]["props"] == [["list", "uchar", "int32", "vertex_indices"]], elements[1]["props"]
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    vertex = np.frombuffer(blob, vdt, nv, end)
    face = np.frombuffer(blob, fdt, nf, end + nv * vdt.itemsize)
    assert (face["n"] == 3).all()
    return dict(vertex=vertex, faces=face["v"].copy(), header=header, payload_bytes=len(blob) - end,
                expected_bytes=nv * vdt.itemsize + nf * fdt.itemsize)


def read_obj(path):
    """`v x y z r g b`, `vn x y z`, `f a//a b//b c//c` -> dict(verts, colors, normals, faces 0-based)"""
    v, vn, f = [], [], []
    for ln in open(path):
        w = ln.split()
        if w[:1] == ["v"]:
            v.append([float(t) for t in w[1:7]])
        elif w[:1] == ["vn"]:
            vn.append([float(t) for t in w[1:4]])
        elif w[:1] == ["f"]:
            f.append([int(t.split("/")[0]) - 1 for t in w[1:4]])
    v = np.array(v).reshape(-1, 6)
    return dict(verts=v[:, :3], colors=v[:, 3:], normals=np.array(vn).reshape(-1, 3), faces=np.array(f, np.int32).reshape(-1, 3))


# ---- test lattices ----------------------------------------------------------------------------------------------------
def sphere_lattice(N, centre=(0.0, 0.0, 0.0), radius=0.6, lo=DEFAULT_BOX[0], hi=DEFAULT_BOX[1], level=10.0, gain=40.0):
    """fp32 lattice of level + gain (radius - |x - centre|): inside the sphere iff above the level"""
    P = lattice_points64(N, lo, hi)
    return (level + gain * (radius - np.linalg.norm(P - np.asarray(centre, np.float64), axis=1))).astype(np.float32)


def two_spheres_lattice(N, level=10.0):
    a = sphere_lattice(N, (-0.45, -0.1, 0.0), 0.4, level=level)
    b = sphere_lattice(N, (0.55, 0.2, 0.1), 0.25, level=level)
    return np.maximum(a, b)


def noise_lattice(N, seed, level=10.0):
    return (level + np.random.RandomState(seed).uniform(-1, 1, N ** 3)).astype(np.float32)
