"""The search index's interface without a GPU: the rgc_search_* symbols are exported from the built library with the header's signatures, a NULL context
or NULL outputs are RGC_ERR_INVALID and no crash, rgc_search_sort_window() is positive (and the window the designed cases are made for), search.KdTree
imports, the C++ adaptor compiles -Wall -Wextra -Werror against the header, the header is still a C99 header, and the generated inventories are current."""
import ctypes as C
import os
import re
import subprocess
import sys

import search_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")
NAMES = ["rgc_search_set_cloud", "rgc_search_clear", "rgc_search_get_info", "rgc_search_sort_window", "rgc_search_knn", "rgc_search_radius"]


def _header_protos():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rgc_hip.h")).read(), flags=re.S)
    return {name: [a.strip() for a in args.split(",")] if args.strip() not in ("", "void") else []
            for name, args in re.findall(r"RGC_API\s+int\s+(rgc_search_\w+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)}


def test_the_symbols_are_exported_with_the_headers_signatures():
    from rgc_slam_amd import _lib
    protos = _header_protos()
    assert sorted(protos) == sorted(NAMES)
    L = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert getattr(raw, name) is not None
        f = getattr(L, name)
        assert len(f.argtypes or []) == len(protos[name]), (name, protos[name], f.argtypes)
        for p, t in zip(protos[name], f.argtypes or []):
            if "*" in p:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, p, t)
            elif "double" in p:
                assert t is C.c_double, (name, p, t)
            elif "long long" in p:
                assert t is C.c_longlong, (name, p, t)
            else:
                assert t is C.c_int, (name, p, t)
    assert [n for n, _ in _lib.SearchInfo._fields_] == ["n", "cell", "cells", "candidates", "grown", "rows_sorted_long"]
    hdr = open(os.path.join(ROOT, "include", "rgc_hip.h")).read()
    assert "#define RGC_SEARCH_MAX_K 32" in hdr and _lib.SEARCH_MAX_K == 32


def test_null_arguments_are_invalid_and_the_window_is_positive():
    from rgc_slam_amd import _lib
    L = _lib.load()
    total = C.c_longlong(-7)
    info = _lib.SearchInfo()
    assert L.rgc_search_set_cloud(None, None, 0, 0, 0, 0.0) == _lib.ERR_INVALID
    assert L.rgc_search_clear(None) == _lib.ERR_INVALID
    assert L.rgc_search_get_info(None, C.byref(info)) == _lib.ERR_INVALID
    assert L.rgc_search_knn(None, None, 0, 0, 0, 0, None, None) == _lib.ERR_INVALID
    assert L.rgc_search_radius(None, None, 0, 0, 0, 0.0, 0, 0, None, None, None, 0, None) == _lib.ERR_INVALID
    assert L.rgc_search_radius(None, None, 0, 0, 0, 1.0, 0, 1, None, None, None, 0, C.byref(total)) == _lib.ERR_INVALID and total.value == -7
    w = L.rgc_search_sort_window()
    assert w > 0 and w == sc.DEFAULT_WINDOW


def test_the_python_mirror_imports():
    import rgc_slam_amd
    from rgc_slam_amd import search
    assert "search" in rgc_slam_amd.__all__
    for name in ("setInputCloud", "nearestKSearch", "radiusSearch", "info", "clear"):
        assert callable(getattr(search.KdTree, name))
    assert search.sort_window() == sc.DEFAULT_WINDOW


def test_the_cpp_adaptor_compiles_and_links(tmp_path):
    out = tmp_path / "test_kdtree"
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_kdtree.cpp"), "-o", str(out),
                           "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    assert out.exists()


def test_the_header_is_still_a_c99_header(tmp_path):
    src = tmp_path / "consumer.c"
    src.write_text('#include "rgc_hip.h"\nint main(void) { rgc_search_info s; s.n = RGC_SEARCH_MAX_K; return rgc_search_sort_window() > 0 && s.n == 32 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "consumer.o")])


def test_the_generated_inventories_are_current():
    for script in ("make_abi_index.py", "make_knobs.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--check"], capture_output=True, text=True)
        assert r.returncode == 0, (script, r.stdout, r.stderr)
