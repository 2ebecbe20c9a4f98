"""ctypes binding of libinstantavatar_hip.so (the C ABI in include/instantavatar_hip.h and its per-feature siblings).

There is NO fallback: if the library is missing or a call fails, this raises.
The headers are the single source of the binding: `build.HEADERS` registers them, `lib()` parses their prototypes
(`parse_header`) into one table and sets every function's restype / argtypes from it, and `call(name, *args)` -- the one
way the package launches a kernel -- marshals its arguments against the same record: tensors as raw device pointers
(checked: on the GPU, contiguous, of the dtype the pointee type admits), descriptor structs by reference, the current
HIP stream when the caller leaves it out.
"""
import collections
import ctypes as C
import os
import re

import torch

from . import build

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libinstantavatar_hip.so")

IA_MAX_LEVELS = 16
IA_N_INIT_MAX = 16


class SnarfGrid(C.Structure):
    _fields_ = [("D", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("offset", C.c_float * 3), ("scale", C.c_float * 3)]


class HashDesc(C.Structure):
    _fields_ = [("n_levels", C.c_int), ("scale", C.c_float * IA_MAX_LEVELS),
                ("res", C.c_uint32 * IA_MAX_LEVELS), ("offset", C.c_uint32 * (IA_MAX_LEVELS + 1))]


class Field(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("scale", C.c_float * 3), ("hash", HashDesc),
                ("table", C.c_void_p), ("sig_w1", C.c_void_p), ("sig_w2", C.c_void_p),
                ("col_w1", C.c_void_p), ("col_w2", C.c_void_p), ("col_w3", C.c_void_p), ("mlp_frags", C.c_void_p),
                ("enc_ws", C.c_void_p), ("enc_ws_samples", C.c_size_t), ("enc_split", C.c_int32)]


class OccGrid(C.Structure):
    _fields_ = [("G", C.c_int), ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3)]


class AdamTensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("shadow", C.c_void_p), ("step", C.c_void_p), ("lr_dev", C.c_void_p),
                ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("numel", C.c_longlong)]


IA_ADAM_MAX_TENSORS = 8


class SmplBody(C.Structure):
    _fields_ = [("v_template", C.c_void_p), ("shapedirs", C.c_void_p), ("posedirs", C.c_void_p), ("lbs_weights", C.c_void_p),
                ("J0", C.c_void_p), ("JS", C.c_void_p), ("parents", C.c_void_p), ("n_verts", C.c_int)]


def header_path(key="main"):
    """Path of the registered C-ABI header `key`.  The registry (`build.HEADERS`) holds one key per header under include/;
    the file name follows from the key (`build.header_name`)."""
    return build.header_path(key)


_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "long": C.c_long,
            "long long": C.c_longlong, "int32_t": C.c_int32}
_RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "const char *": C.c_char_p}
_STRUCTS = {"ia_snarf_grid": SnarfGrid, "ia_hash_desc": HashDesc, "ia_field": Field, "ia_occ_grid": OccGrid,
            "ia_adam_tensor": AdamTensor, "ia_smpl_body": SmplBody}
# Pointee type -> the dtypes a tensor handed to `call` for such a parameter may have (None: any), fixed from what the call
# sites pass.  Every pointer to a scalar binds as c_void_p (device tensors and host arrays alike); the pointee only feeds this check.
#   uint8_t   uint8, and bool: the one parameter kind that legitimately receives two dtypes -- DensityGrid's occ_bool outputs are
#             bool tensors whose bytes 0 / 1 the kernels write
#   uint16_t  float16: the header's fp16 convention
#   uint32_t  int32: the occupancy bits, the encoder planes and the grad-scale state are allocated as int32 words
#   double, int, uint64_t  no tensor at all: HOST arrays (ia_make_rays, the profile getters), given as ctypes objects
_POINTEES = {"float": (torch.float32,), "int32_t": (torch.int32,), "int64_t": (torch.int64,), "long long": (torch.int64,),
             "uint8_t": (torch.uint8, torch.bool), "uint16_t": (torch.float16,), "uint32_t": (torch.int32,), "void": None,
             "double": (), "int": (), "uint64_t": ()}

#: one parameter of a prototype.  kind: "scalar" | "pointer" (to a scalar or void; `of` = admitted dtypes) |
#: "struct" (`of` = the ctypes mirror) | "str"
Param = collections.namedtuple("Param", "name ctype kind of")
Decl = collections.namedtuple("Decl", "restype params stream")   # stream: the last parameter is `void *stream`


def parse_header(text):
    """{function name: Decl} of every prototype in the text of include/instantavatar_hip.h.  Not a C parser: the header
    holds comments, preprocessor lines, `typedef struct {...} name;` and `ret name(type [*]param, ...);` over the types of
    the tables above, and anything else -- a type that is not in them, a function pointer, an array parameter -- raises."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r"typedef\s+struct\s+\w*\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    text = re.sub(r'extern\s+"C"\s*\{|\}', " ", text)
    decls = {}
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        m = re.fullmatch(r"(int|size_t|const char \*) ?(\w+) ?\((.*)\)", stmt)
        if not m:
            raise ImportError("instantavatar_hip.h: cannot parse the declaration `%s`" % stmt)
        ret, fname, arglist = m.groups()
        params = []
        for arg in ([] if arglist.strip() in ("", "void") else arglist.split(",")):
            a = re.fullmatch(r"\s*(const )?([\w ]+?) ?(\*?) ?(\w+)\s*", arg)
            const, base, star, pname = a.groups() if a else (None, None, None, None)
            if not star and base in _SCALARS:
                params.append(Param(pname, _SCALARS[base], "scalar", None))
            elif star and base in _STRUCTS:
                params.append(Param(pname, C.POINTER(_STRUCTS[base]), "struct", _STRUCTS[base]))
            elif star and base in _POINTEES:
                params.append(Param(pname, C.c_void_p, "pointer", _POINTEES[base]))
            elif star and const and base == "char":
                params.append(Param(pname, C.c_char_p, "str", None))
            else:
                raise ImportError("instantavatar_hip.h: %s: cannot classify the parameter `%s`" % (fname, arg.strip()))
        stream = bool(params) and params[-1].name == "stream" and params[-1].of is None and params[-1].kind == "pointer"
        decls[fname] = Decl(_RETURNS[ret], tuple(params), stream)
    return decls


def _parse_file(path):
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise ImportError("instantavatar_amd: the C header %s is missing (%s); the binding is derived from it"
                          % (os.path.normpath(path), e))
    return parse_header(text)


_decls = {}      # header key -> its table, filled by `declarations`


def declarations(key="main"):
    """parse_header of this checkout's registered header `key`, read once.  Without a key: the main header's table."""
    d = _decls.get(key)
    if d is None:
        d = _decls[key] = _parse_file(header_path(key))
    return d


def merge_tables(tables):
    """One {function name: Decl} out of `(header file name, table)` pairs, in their order.  A name that two headers declare
    is an error that names both of them."""
    merged, owner = {}, {}
    for fname, table in tables:
        for name, d in table.items():
            if name in owner:
                raise ImportError("%s declares %s, which %s declares already" % (fname, name, owner[name]))
            owner[name] = fname
            merged[name] = d
    return merged


def merged_table():
    """The prototypes of every registered header, in registry order: what `lib()` binds and `call` reaches."""
    return merge_tables((build.header_name(k), declarations(k)) for k in build.HEADERS)


def __getattr__(name):
    if name == "EXPORTED":       # the sorted names of the declared functions
        return sorted(declarations())
    raise AttributeError(name)


_Tensor, _Structure = torch.Tensor, C.Structure     # (module-level names: `call` looks them up per argument)
_lib = None
_bound = {}      # name -> (ctypes function, its pointer parameters, parameter count, ends in `void *stream`, returns int): for `call`


def lib():
    """Load the HIP library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "instantavatar_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback." % LIB_PATH)
        # a library built from other sources than this checkout is an error, not something to run silently (edit a kernel,
        # forget to rebuild, and every number is the OLD kernel's).  The manifest is read from the file's bytes; variants
        # built with IA_EXTRA_HIPCC_FLAGS carry the flags in their hashes, so the same variable must be set when they run.
        if os.environ.get("IA_ALLOW_STALE_LIB", "0") != "1":
            have = build.library_manifest(LIB_PATH)
            try:
                want = build.source_manifest()
            except OSError:      # a csrc/ without the shared headers: nothing to compare against
                want = {}
            # (an installation that ships the library without its sources -- a wheel, a container layer -- has nothing to be
            # stale against: the check only applies where there is a checkout to have edited)
            if want and have != want:
                diff = sorted(k for k in set(have) | set(want) if have.get(k) != want.get(k))
                raise ImportError(
                    "instantavatar_amd: %s was built from other sources than this checkout (differs in: %s). Rebuild it "
                    "(`python -m instantavatar_amd.build`), or set IA_ALLOW_STALE_LIB=1 to run it anyway." % (LIB_PATH, ", ".join(diff)))
        l = C.CDLL(LIB_PATH)
        for name, d in merged_table().items():
            fn = getattr(l, name)  # AttributeError if a symbol is missing
            fn.restype = d.restype
            fn.argtypes = [p.ctype for p in d.params]
            # what `call` does per pointer parameter: (index, name, admitted dtypes, struct); a struct parameter admits no tensor
            ptrs = tuple((i, p.name, (), p.of) if p.kind == "struct" else (i, p.name, p.of, None)
                         for i, p in enumerate(d.params[:-1] if d.stream else d.params) if p.kind in ("pointer", "struct"))
            _bound[name] = (fn, ptrs, len(d.params), d.stream, d.restype is C.c_int)
        _lib = l
    return _lib


class IAError(RuntimeError):
    pass


def check(rc, what=""):
    if rc != 0:
        msg = lib().ia_last_error()
        raise IAError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))


def ptr(t):
    """Device pointer of a contiguous tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous(), "tensor must be contiguous"
    return t.data_ptr()


def scratch(owner, name, nbytes, device):
    """A byte buffer of at least `nbytes` cached on `owner` under `name` (grown, never shrunk): the caller-provided
    workspaces of the C ABI.  Sized during the eager warm-up calls, so a captured graph replays with fixed pointers."""
    t = getattr(owner, name, None)
    if t is None or t.numel() < nbytes or t.device != torch.device(device):
        t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
        setattr(owner, name, t)
    return t


def stream():
    """Raw handle of torch's current stream on the current device (the one kernels are launched on; inside
    `torch.cuda.graph` it is the capturing stream).  The raw getter costs ~0.3 us, `torch.cuda.current_stream()`
    ~12 us -- nine calls per training step."""
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise IAError("instantavatar_amd kernels need tensors on the GPU (got %s); there is no CPU path" % t.device)


def _reject(name, pname, why):
    raise IAError("%s: argument `%s` %s" % (name, pname, why))


def _reject_tensor(name, pname, t, dtypes, struct):
    if struct is not None:
        _reject(name, pname, "is a tensor where a %s is declared" % struct.__name__)
    if not t.is_cuda:
        _reject(name, pname, "must be on the GPU (got %s); there is no CPU path" % t.device)
    if not t.is_contiguous():
        _reject(name, pname, "must be contiguous (got strides %s for shape %s)" % (tuple(t.stride()), tuple(t.shape)))
    _reject(name, pname, "is %s where the header admits %s" % (t.dtype, " / ".join(map(str, dtypes)) or "no tensor (a host array)"))


def call(name, *args):
    """Call the C-ABI function `name` with `args` marshalled against its prototype in the header:

      pointer parameter   a tensor (its data_ptr(), after checking that it is on the GPU, contiguous and of a dtype the
                          pointee admits, see _POINTEES), None (NULL), an int (a raw device address: sub-buffers), a descriptor
                          struct (passed by reference), or any other ctypes object (host arrays, byref(...)) as it is
      scalar parameter    a Python number
      void *stream        may be left out as the last argument: the current stream (`stream()`)

    A wrong argument count or a failed tensor check raises IAError naming the function and the parameter, before
    anything is launched.  Functions that return a status raise through `check` when it is negative; the others
    (`*_bytes`, ia_field_act_stride, ia_version) return their value.

    Lifetime: `args` holds every tensor, temporaries included, until the function has returned, i.e. until the launch is
    enqueued; a block the allocator hands out again after that is reused in stream order behind the kernel, which is
    safe on the same stream.  (Not so for a temporary given to `ptr()`: it dies before the launch.)"""
    f = _bound.get(name)
    if f is None:
        lib()
        f = _bound.get(name)
        if f is None:
            files = [build.header_name(k) for k in build.HEADERS]
            raise IAError("%s is not declared in include/%s (nor in %s)" % (name, files[0], " / ".join(files[1:])))
    fn, ptrs, n, has_stream, int_ret = f
    if len(args) != n:
        if has_stream and len(args) == n - 1:
            args += (stream(),)
        else:
            raise IAError("%s takes %d arguments%s, got %d" % (name, n, " (the trailing stream may be left out)" if has_stream else "", len(args)))
    if ptrs:
        out = list(args)
        for i, pname, dtypes, struct in ptrs:
            a = out[i]
            if isinstance(a, _Tensor):
                if a.is_cuda and a.is_contiguous() and (dtypes is None or a.dtype in dtypes):
                    out[i] = a.data_ptr()
                else:
                    _reject_tensor(name, pname, a, dtypes, struct)
            elif isinstance(a, _Structure):
                if type(a) is not struct:
                    _reject(name, pname, "is a %s where %s is declared" % (type(a).__name__, struct.__name__ if struct else "a pointer to scalars"))
                out[i] = C.byref(a)
        rc = fn(*out)
    else:
        rc = fn(*args)
    if int_ret and rc < 0:
        check(rc, name)
    return rc


def bone_array(bone_ids):
    arr = (C.c_int32 * len(bone_ids))(*[int(b) for b in bone_ids])
    return arr


def apply_level3_override(hd, n_levels, log2_hashmap_size, level3_res=None):
    """tcnn derives a level's resolution as ceil(exp2f(l * log2f(1.5)) * 16 - 1) + 1.  For l = 3 the exact value of
    the scale is 53.0, so the result is 54 or 55 depending on the last bit of the exp2f in use (glibc: 54; a libm or
    device intrinsic that returns 3.3750002 gives 55) -- which one the reference's tcnn v1.6 build produced cannot be
    decided without one of its checkpoints.  `level3_res` (or the environment variable IA_TCNN_LEVEL3_RES, so that the
    whole test suite can be run under either) selects the layout explicitly; offsets are recomputed with tcnn's rule
    (entries = min(round_up(res^3, 8), 2^log2_hashmap_size))."""
    import os
    if level3_res is None:
        level3_res = os.environ.get("IA_TCNN_LEVEL3_RES")
    if level3_res is None or n_levels <= 3:
        return hd
    level3_res = int(level3_res)
    if level3_res not in (54, 55):
        raise ValueError("IA_TCNN_LEVEL3_RES / level3_res must be 54 or 55, got %r" % (level3_res,))
    hd.res[3] = level3_res
    off = 0
    for l in range(n_levels):
        r = int(hd.res[l])
        n = min((r * r * r + 7) // 8 * 8, 1 << log2_hashmap_size)
        hd.offset[l] = off
        off += n
    hd.offset[n_levels] = off
    return hd


def make_hash_desc(n_levels=16, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.5, level3_res=None):
    hd = HashDesc()
    call("ia_hash_desc_init", hd, n_levels, log2_hashmap_size, base_resolution, per_level_scale)
    return apply_level3_override(hd, n_levels, log2_hashmap_size, level3_res)
