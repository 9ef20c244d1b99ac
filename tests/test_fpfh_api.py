"""The FPFH descriptors' interface without a GPU, after tests/test_normals_api.py: the rgc_fpfh_* symbols are exported from the built library with the header's
signatures, the ctypes structures mirror rgc_fpfh_params and rgc_fpfh_info field by field (names, sizeof and offsets against the C compiler), the default radius
is 0 (a caller must choose), the refusals that need no context (a NULL context, NULL params / n_valid, a NULL info) are RGC_ERR_INVALID with no crash and no
output touched -- the range refusals of a live context are in tests/test_gpu_fpfh.py, which has one --, the header block carries [3P-memory], the pair term and
every listed deviation, features.FPFHEstimation imports with PCL's member names and its setter refuses what the C-ABI would, Preprocessor carries the member,
the C++ adaptor compiles -Wall -Wextra -Werror against the header, the header is still a C99 header, both new files are in the build, and the generated
inventories are current."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")
NAMES = {"rgc_default_fpfh_params": 1, "rgc_fpfh_estimate": 16, "rgc_fpfh_get_info": 2, "rgc_fpfh_set_cell": 2}
PARAM_FIELDS = ["radius", "reserved"]
INFO_FIELDS = ["n", "n_surface", "n_valid", "n_spfh", "cell", "cells", "pairs", "candidates", "reserved"]
SENTINEL = -77


def _header_protos():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rgc_hip.h")).read(), flags=re.S)
    return {name: [a.strip() for a in args.split(",")] if args.strip() not in ("", "void") else []
            for name, args in re.findall(r"RGC_API\s+(?:int|void)\s+(rgc_(?:default_)?fpfh_\w+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)}


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
    block = hdr[hdr.index("FPFH descriptors: pcl::FPFHEstimation"):hdr.index("typedef struct rgc_fpfh_params")]
    assert "[3P-memory]" in block and "do not call the PCL class" in block
    for said in ("fp64 pair terms where PCL uses fp32", "the swap test on the numerators where PCL compares acosf values", "the strict radius rule", "key < r2",
                 "invalid normals skipped pair by pair", "the k route", "the indices subset", "setNrSubdivisions other than 11 / 11 / 11", "FPFHEstimationOMP",
                 "SAC-IA / prerejective alignment", "MAY DEPEND ON THE CELL SIZE", "Swap iff |c1| < |c2|, strict", "skipped if vn == 0", "f1 = atan2(", "clamped to 0..10",
                 "inc_s = 100.0 / (double)(m_s - 1)", "w_j = 1.0 / (double)key_j", "the query's own normal is never read", "33 quiet NaNs", "-1 (with a row of zeros)",
                 "RGC_ERR_NONFINITE", "RGC_ERR_GRID_TOO_LARGE", "A solve in flight refuses the call", "not re-normalised", "info.n_spfh", "no floating-point atomic"):
        assert said in block, said


def test_the_structures_match_the_compilers_layout_and_the_default_radius_is_zero(tmp_path):
    from rgc_slam_amd import _lib
    assert [n for n, _ in _lib.FpfhParams._fields_] == PARAM_FIELDS and [n for n, _ in _lib.FpfhInfo._fields_] == INFO_FIELDS
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "rgc_hip.h"', "int main(void) {", '  printf("%zu", sizeof(rgc_fpfh_params));']
    src += ['  printf(" %%zu", offsetof(rgc_fpfh_params, %s));' % f for f in PARAM_FIELDS] + ['  printf("\\n%zu", sizeof(rgc_fpfh_info));']
    src += ['  printf(" %%zu", offsetof(rgc_fpfh_info, %s));' % f for f in INFO_FIELDS]
    src += ['  printf("\\n%d\\n", RGC_FPFH_BINS);', "  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    lines = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines()
    for cls, fields, line in ((_lib.FpfhParams, PARAM_FIELDS, lines[0]), (_lib.FpfhInfo, INFO_FIELDS, lines[1])):
        size, *offs = line.split()
        assert C.sizeof(cls) == int(size) and [getattr(cls, f).offset for f in fields] == [int(o) for o in offs], cls
    assert int(lines[2]) == _lib.FPFH_BINS == 33
    p = _lib.FpfhParams(radius=3.0)
    p.reserved[0] = 9
    _lib.load().rgc_default_fpfh_params(C.byref(p))
    assert (p.radius, list(p.reserved)) == (0.0, [0, 0])                         # a caller must choose
    _lib.load().rgc_default_fpfh_params(None)                                    # no crash


def test_context_free_refusals_leave_every_output_alone():
    from rgc_slam_amd import _lib
    L = _lib.load()
    cloud, normals = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32)
    out, spfh = np.full((4, 33), SENTINEL, np.float32), np.full((4, 33), 77, np.uint32)
    scnt, cnt = np.full(4, SENTINEL, np.int32), np.full(4, SENTINEL, np.int32)
    valid = C.c_int(SENTINEL)
    prm = _lib.FpfhParams(radius=0.5)
    call = lambda ctx, p, v: L.rgc_fpfh_estimate(ctx, cloud.ctypes.data, 4, 12, None, 0, 0, normals.ctypes.data, 12, 0, p, out.ctypes.data, spfh.ctypes.data, scnt.ctypes.data,
                                                 cnt.ctypes.data, v)
    assert call(None, C.byref(prm), C.byref(valid)) == _lib.ERR_INVALID and call(None, None, None) == _lib.ERR_INVALID
    info = _lib.FpfhInfo()
    assert L.rgc_fpfh_get_info(None, C.byref(info)) == _lib.ERR_INVALID and L.rgc_fpfh_set_cell(None, 0.0) == _lib.ERR_INVALID
    assert (out == SENTINEL).all() and (spfh == 77).all() and (scnt == SENTINEL).all() and (cnt == SENTINEL).all() and valid.value == SENTINEL


def test_the_python_mirror_has_pcls_member_names_and_its_setter_refuses():
    from rgc_slam_amd import features as ft, odometry
    for name in ("setInputCloud", "setSearchSurface", "setInputNormals", "setRadiusSearch", "getRadiusSearch", "compute", "getSPFH", "getCounts", "getValidCount", "info", "setCell"):
        assert callable(getattr(ft.FPFHEstimation, name)), name
    assert callable(odometry.Preprocessor.fpfhEstimation)
    s = object.__new__(ft.FPFHEstimation)                    # (no device is opened here)
    s._init_params()
    assert s.getRadiusSearch() == 0.0 and s.getSPFH() == (None, None) and s.getCounts() is None and s.getValidCount() is None
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-30, 1e30):
        with pytest.raises(ft.RgcError):
            s.setRadiusSearch(bad)
    with pytest.raises(ft.RgcError):
        s.compute()                                          # no input cloud: refused before any context is touched
    s.setInputCloud(np.zeros((4, 3), np.float32))
    with pytest.raises(ft.RgcError):
        s.compute()                                          # no normals
    s.setInputNormals(np.zeros((4, 3), np.float32))
    with pytest.raises(ft.RgcError):
        s.compute()                                          # no radius chosen
    s.setRadiusSearch(0.5)
    assert s.getRadiusSearch() == 0.5


def test_the_cpp_adaptor_compiles_and_links(tmp_path):
    out = tmp_path / "test_fpfh"
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_fpfh.cpp"), "-o", str(out),
                           "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    assert out.exists()
    hpp = open(os.path.join(PKG, "cpp", "features_hip.hpp")).read()
    for name in ("class FPFHEstimationHip", "setInputCloud", "setSearchSurface", "setInputNormals", "setRadiusSearch", "getRadiusSearch", "setCell",
                 "int compute(std::vector<float>& fpfh)", "computeDevice", "setInputDevice"):
        assert name in hpp[hpp.index("class FPFHEstimationHip"):], name


def test_the_header_is_still_a_c99_header(tmp_path):
    src = tmp_path / "consumer.c"
    src.write_text('#include "rgc_hip.h"\nint main(void) { rgc_fpfh_params p; rgc_fpfh_info s; float f[RGC_FPFH_BINS]; float nr[3] = {0, 0, 1}; int m = 0; rgc_default_fpfh_params(&p); s.n = 3;\n'
                   '  return rgc_fpfh_set_cell(0, 0.0) == RGC_ERR_INVALID && rgc_fpfh_get_info(0, &s) == RGC_ERR_INVALID &&\n'
                   '         rgc_fpfh_estimate(0, 0, 0, 12, 0, 0, 0, nr, 12, 0, &p, f, 0, 0, 0, &m) == RGC_ERR_INVALID && s.n == 3 && p.radius == 0.0 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "consumer.o")])


def test_both_files_are_in_the_build_and_the_inventories_are_current():
    build = open(os.path.join(PKG, "build.py")).read()
    assert '"rgc_fpfh.hip"' in build and '"rgc_api_fpfh.hip"' in build
    for script in ("make_abi_index.py", "make_knobs.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--check"], capture_output=True, text=True)
        assert r.returncode == 0, (script, r.stdout, r.stderr)
