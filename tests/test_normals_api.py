"""Surface normal estimation's interface without a GPU, after tests/test_plane_api.py: the rgc_normal_* symbols are exported from the built library with the
header's signatures, the ctypes structures mirror rgc_normal_params and rgc_normal_info field by field (names, sizeof and offsets against the C compiler),
the defaults are PCL's (no route chosen, flip on, the viewpoint at the origin), the refusals that need no context (a NULL context, NULL params / n_valid, a NULL
info) are RGC_ERR_INVALID with no crash and no output touched -- the range refusals of a live context are in tests/test_gpu_normals.py, which has one --, the
header block carries [3P-memory] and every listed deviation, features.NormalEstimation imports with PCL's member names and its setters refuse what the C-ABI
would, Preprocessor carries the member, the C++ adaptor compiles -Wall -Wextra -Werror against the header, the header is still a C99 header, both new files
are in the build, and the generated inventories are current."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")
NAMES = {"rgc_default_normal_params": 1, "rgc_normal_estimate": 14, "rgc_normal_get_info": 2, "rgc_normal_set_cell": 2}
PARAM_FIELDS = ["k", "flip", "radius", "viewpoint", "reserved"]
INFO_FIELDS = ["n", "n_surface", "n_valid", "route", "cell", "cells", "candidates", "grown", "reserved"]
SENTINEL = -77


def _header_protos():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rgc_hip.h")).read(), flags=re.S)
    return {name: [a.strip() for a in args.split(",")] if args.strip() not in ("", "void") else []
            for name, args in re.findall(r"RGC_API\s+(?:int|void)\s+(rgc_(?:default_)?normal_\w+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)}


def test_the_symbols_are_exported_with_the_headers_signatures():
    from rgc_slam_amd import _lib
    protos = _header_protos()
    assert sorted(protos) == sorted(NAMES)
    L = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name, nargs in NAMES.items():
        assert getattr(raw, name) is not None and name in _lib.SYMBOLS and len(protos[name]) == nargs
        f = getattr(L, name)
        assert len(f.argtypes or []) == nargs, (name, protos[name], f.argtypes)
        for p, t in zip(protos[name], f.argtypes):
            if "*" in p:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, p, t)
            elif "double" in p:
                assert t is C.c_double, (name, p, t)
            else:
                assert t is C.c_int, (name, p, t)


def test_the_header_block_states_the_semantics_and_every_deviation():
    hdr = open(os.path.join(ROOT, "include", "rgc_hip.h")).read()
    block = hdr[hdr.index("surface normal estimation: pcl::NormalEstimation"):hdr.index("typedef struct rgc_normal_params")]
    assert "[3P-memory]" in block and "do not call the PCL class" in block
    for said in ("fp64 moments about the query where PCL sums fp32 unshifted", "the strict radius rule", "the tie rule of equal eigenvalues", "the sign of an exact 0",
                 "the flip = 0 sign rule", "the indices subset", "OMP and integral-image variants", "PointNormal output packing", "ascending (key, index)",
                 "MAY DEPEND ON THE CELL SIZE", "normalises by the count m and not", "an exact 0 keeps the sign", "four quiet NaNs", "RGC_ERR_NONFINITE", "RGC_ERR_GRID_TOO_LARGE",
                 "key < r2, STRICT", "A solve in flight refuses the call"):
        assert said in block, said


def test_the_structures_match_the_compilers_layout_and_the_defaults_are_pcls(tmp_path):
    from rgc_slam_amd import _lib
    assert [n for n, _ in _lib.NormalParams._fields_] == PARAM_FIELDS and [n for n, _ in _lib.NormalInfo._fields_] == INFO_FIELDS
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "rgc_hip.h"', "int main(void) {", '  printf("%zu", sizeof(rgc_normal_params));']
    src += ['  printf(" %%zu", offsetof(rgc_normal_params, %s));' % f for f in PARAM_FIELDS] + ['  printf("\\n%zu", sizeof(rgc_normal_info));']
    src += ['  printf(" %%zu", offsetof(rgc_normal_info, %s));' % f for f in INFO_FIELDS]
    src += ['  printf("\\n%d %d %d\\n", RGC_NORMAL_MAX_K, RGC_NORMAL_ROUTE_K, RGC_NORMAL_ROUTE_RADIUS);', "  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    lines = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines()
    for cls, fields, line in ((_lib.NormalParams, PARAM_FIELDS, lines[0]), (_lib.NormalInfo, INFO_FIELDS, lines[1])):
        size, *offs = line.split()
        assert C.sizeof(cls) == int(size) and [getattr(cls, f).offset for f in fields] == [int(o) for o in offs], cls
    assert [int(v) for v in lines[2].split()] == [_lib.NORMAL_MAX_K, _lib.NORMAL_ROUTE_K, _lib.NORMAL_ROUTE_RADIUS]
    p = _lib.NormalParams(k=9, flip=0, radius=3.0)
    _lib.load().rgc_default_normal_params(C.byref(p))
    assert (p.k, p.radius, p.flip, list(p.viewpoint), p.reserved) == (0, 0.0, 1, [0.0, 0.0, 0.0], 0)      # a caller must choose a route, as in PCL
    _lib.load().rgc_default_normal_params(None)                                   # no crash


def test_context_free_refusals_leave_every_output_alone():
    from rgc_slam_amd import _lib
    L = _lib.load()
    cloud = np.zeros((4, 3), np.float32)
    n4, cov, cen, cnt = np.full((4, 4), SENTINEL, np.float32), np.full((4, 6), float(SENTINEL)), np.full((4, 3), float(SENTINEL)), np.full(4, SENTINEL, np.int32)
    valid = C.c_int(SENTINEL)
    prm = _lib.NormalParams()
    L.rgc_default_normal_params(C.byref(prm))
    prm.k = 3
    call = lambda ctx, p, v: L.rgc_normal_estimate(ctx, cloud.ctypes.data, 4, 12, None, 0, 0, 0, p, n4.ctypes.data, cov.ctypes.data, cen.ctypes.data, cnt.ctypes.data, v)
    assert call(None, C.byref(prm), C.byref(valid)) == _lib.ERR_INVALID and call(None, None, None) == _lib.ERR_INVALID
    info = _lib.NormalInfo()
    assert L.rgc_normal_get_info(None, C.byref(info)) == _lib.ERR_INVALID and L.rgc_normal_set_cell(None, 0.0) == _lib.ERR_INVALID
    assert (n4 == SENTINEL).all() and (cov == SENTINEL).all() and (cen == SENTINEL).all() and (cnt == SENTINEL).all() and valid.value == SENTINEL


def test_the_python_mirror_has_pcls_member_names_and_its_setters_refuse():
    import rgc_slam_amd
    from rgc_slam_amd import features as ft, odometry
    assert "features" in rgc_slam_amd.__all__
    for name in ("setInputCloud", "setSearchSurface", "setKSearch", "getKSearch", "setRadiusSearch", "getRadiusSearch", "setViewPoint", "getViewPoint", "compute", "setFlip",
                 "setCell", "info", "getCovariances", "getCentroids", "getCounts", "getValidCount"):
        assert callable(getattr(ft.NormalEstimation, name)), name
    assert callable(odometry.Preprocessor.normalEstimation)
    s = object.__new__(ft.NormalEstimation)                  # (no device is opened here)
    s._init_params()
    assert (s.getKSearch(), s.getRadiusSearch(), s.getViewPoint()) == (0, 0.0, (0.0, 0.0, 0.0))
    for setter, bads in ((s.setKSearch, (1, 2, 33, -1)), (s.setRadiusSearch, (-1.0, float("nan"), float("inf"), 1e-30, 1e30)),
                         (lambda v: s.setViewPoint(*v), ((float("nan"), 0, 0), (0, float("inf"), 0), (0, 0, 1e39)))):
        for bad in bads:
            with pytest.raises(ft.RgcError):
                setter(bad)
    s.setKSearch(10)
    assert (s.getKSearch(), s.getRadiusSearch()) == (10, 0.0)
    s.setRadiusSearch(0.5)                                   # the one route deselects the other
    assert (s.getKSearch(), s.getRadiusSearch()) == (0, 0.5)
    s.setKSearch(32)
    s.setViewPoint(1.0, -2.0, 0.1)
    assert (s.getKSearch(), s.getRadiusSearch(), s.getViewPoint()) == (32, 0.0, (1.0, -2.0, float(np.float32(0.1))))
    with pytest.raises(ft.RgcError):
        s.compute()                                          # no input cloud: refused before any context is touched
    s.setInputCloud(np.zeros((4, 3), np.float32))
    s.setKSearch(0)
    with pytest.raises(ft.RgcError):
        s.compute()                                          # no route chosen


def test_the_cpp_adaptor_compiles_and_links(tmp_path):
    out = tmp_path / "test_normals"
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_normals.cpp"), "-o", str(out),
                           "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    assert out.exists()
    hpp = open(os.path.join(PKG, "cpp", "features_hip.hpp")).read()
    for name in ("class NormalEstimationHip", "setInputCloud", "setSearchSurface", "setKSearch", "setRadiusSearch", "setViewPoint", "getViewPoint", "setFlip", "setCell",
                 "int compute(std::vector<float>& normal4)", "computeDevice"):
        assert name in hpp, name


def test_the_header_is_still_a_c99_header(tmp_path):
    src = tmp_path / "consumer.c"
    src.write_text('#include "rgc_hip.h"\nint main(void) { rgc_normal_params p; rgc_normal_info s; float n4[4]; int m = 0; rgc_default_normal_params(&p); s.n = 3; p.k = RGC_NORMAL_MAX_K;\n'
                   '  return rgc_normal_set_cell(0, 0.0) == RGC_ERR_INVALID && rgc_normal_get_info(0, &s) == RGC_ERR_INVALID &&\n'
                   '         rgc_normal_estimate(0, 0, 0, 12, 0, 0, 0, 0, &p, n4, 0, 0, 0, &m) == RGC_ERR_INVALID && s.n == 3 && p.flip == 1 && RGC_NORMAL_ROUTE_RADIUS == 1 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "consumer.o")])


def test_both_files_are_in_the_build_and_the_inventories_are_current():
    build = open(os.path.join(PKG, "build.py")).read()
    assert '"rgc_normals.hip"' in build and '"rgc_api_normals.hip"' in build
    for script in ("make_abi_index.py", "make_knobs.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--check"], capture_output=True, text=True)
        assert r.returncode == 0, (script, r.stdout, r.stderr)
