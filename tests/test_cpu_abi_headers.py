"""The registry of C-ABI headers (`build.HEADERS`) and what is derived from it: every header under include/ is one key, is part
of every translation unit's source hash, is parsed into one table of `_lib.declarations(key)`, and all of them are merged, with
pairwise disjoint names, into what `_lib.lib()` binds.  What is particular to one header (its names, stream flags, `#define`s)
is in that feature's own test file.  No GPU."""
import glob
import itertools
import os
import re

import pytest

from instantavatar_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_norm = lambda paths: [os.path.normpath(os.path.abspath(p)) for p in paths]


def test_registry_keys_and_file_names():
    assert build.HEADERS == ("main", "io", "normals", "mesh", "raster", "keypoints", "silhouette", "masks", "overlay", "meshops", "texture",
                             "rig", "meshdist", "phototex", "scene", "meshray", "scene_receive", "render_iter", "scene_deep", "png", "lpips")
    assert len(set(build.HEADERS)) == len(build.HEADERS)
    assert build.header_name("main") == "instantavatar_hip.h" and build.header_name("scene_deep") == "instantavatar_hip_scene_deep.h"
    assert os.path.normpath(_lib.header_path()) == os.path.normpath(os.path.join(ROOT, "include", "instantavatar_hip.h"))
    with pytest.raises(KeyError, match="not a registered"):
        _lib.header_path("no_such_header")
    with pytest.raises(KeyError, match="not a registered"):
        _lib.declarations("no_such_header")


def test_shared_headers_are_the_common_header_then_the_registry_in_order():
    assert os.path.normpath(build.SHARED_HEADERS[0]) == os.path.normpath(os.path.join(build.CSRC, "ia_common.h"))
    assert _norm(build.SHARED_HEADERS[1:]) == _norm(_lib.header_path(k) for k in build.HEADERS)
    assert [os.path.basename(h) for h in build.SHARED_HEADERS[1:]] == [build.header_name(k) for k in build.HEADERS]


def test_every_header_on_disk_is_registered():
    on_disk = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert on_disk == sorted(build.header_name(k) for k in build.HEADERS)


def test_every_public_header_the_sources_include_is_registered():
    registered = {build.header_name(k) for k in build.HEADERS}
    found = set()
    for path in sorted(glob.glob(os.path.join(build.CSRC, "*"))):
        if path.endswith((".hip", ".cpp", ".h", ".inc")):
            with open(path) as f:
                for name in re.findall(r'^\s*#\s*include\s+"\.\./\.\./include/([^"]+)"', f.read(), re.M):
                    assert name in registered, "%s includes %s, which build.HEADERS does not register" % (os.path.basename(path), name)
                    found.add(name)
    assert found == registered          # and no registered header is declared for nothing


@pytest.mark.parametrize("key", build.HEADERS)
def test_header_is_hashed_exported_and_bound(key):
    assert _norm([_lib.header_path(key)])[0] in _norm(build.SHARED_HEADERS)
    d = _lib.declarations(key)
    assert d and _lib.declarations(key) is d          # parsed once
    L = _lib.lib()
    for name, decl in d.items():
        assert hasattr(L, name), "%s declares %s, which the library does not export" % (build.header_name(key), name)
        assert name in _lib._bound, name
        assert len(getattr(L, name).argtypes) == len(decl.params) == _lib._bound[name][2], name
        assert _lib._bound[name][3] == decl.stream, name


def test_the_headers_names_are_pairwise_disjoint_and_the_merged_table_holds_them_all():
    for a, b in itertools.combinations(build.HEADERS, 2):
        both = set(_lib.declarations(a)) & set(_lib.declarations(b))
        assert not both, "%s and %s both declare %s" % (build.header_name(a), build.header_name(b), sorted(both))
    merged = _lib.merged_table()
    assert list(merged) == [n for k in build.HEADERS for n in _lib.declarations(k)]          # registry order, then header order
    assert all(merged[n] is _lib.declarations(k)[n] for k in build.HEADERS for n in _lib.declarations(k))
    _lib.lib()
    assert set(_lib._bound) == set(merged)
    assert len(_lib.declarations()) == 89 and _lib.EXPORTED == sorted(_lib.declarations("main"))


def test_merge_refuses_a_duplicate_and_names_both_files():
    a = _lib.parse_header("int ia_one(int n);\nint ia_two(int n);")
    b = _lib.parse_header("int ia_three(int n);")
    c = _lib.parse_header("int ia_four(int n);\nint ia_two(float x);")
    assert list(_lib.merge_tables([("a.h", a), ("b.h", b)])) == ["ia_one", "ia_two", "ia_three"]
    assert _lib.merge_tables([]) == {}
    with pytest.raises(ImportError) as e:
        _lib.merge_tables([("a.h", a), ("b.h", b), ("c.h", c)])
    msg = str(e.value)
    assert "ia_two" in msg and "a.h" in msg and "c.h" in msg and "b.h" not in msg
    assert msg.index("c.h") < msg.index("a.h")          # "<later> declares <name>, which <earlier> declares already"


def test_an_undeclared_name_is_refused_with_every_headers_file_name():
    with pytest.raises(_lib.IAError) as e:
        _lib.call("ia_no_such_function")
    msg = str(e.value)
    assert msg.startswith("ia_no_such_function is not declared in include/instantavatar_hip.h (nor in instantavatar_hip_io.h / ")
    for key in build.HEADERS:
        assert build.header_name(key) in msg, key
