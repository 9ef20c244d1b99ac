"""The outlier filters' interface without a GPU: the rgc_outlier_* symbols are exported from the built library with the header's signatures, the ctypes
structure mirrors rgc_outlier_info field by field (names, sizeof and offsets against the C compiler), a NULL context or a NULL n_out is RGC_ERR_INVALID and no
crash, filters.StatisticalOutlierRemoval / RadiusOutlierRemoval import with PCL's member names and their setters refuse what the C-ABI would, Preprocessor
carries the two members, the C++ adaptors compile -Wall -Wextra -Werror against the header, the header is still a C99 header, the kernels' file is in the
build, and the generated inventories are current."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")
NAMES = ["rgc_outlier_statistical", "rgc_outlier_radius", "rgc_outlier_get_info", "rgc_outlier_set_cell"]
FIELDS = ["n", "n_out", "mean", "stddev", "threshold", "cell", "cells", "candidates", "grown"]


def _header_protos():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rgc_hip.h")).read(), flags=re.S)
    return {name: [a.strip() for a in args.split(",")] if args.strip() not in ("", "void") else []
            for name, args in re.findall(r"RGC_API\s+int\s+(rgc_outlier_\w+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)}


def test_the_symbols_are_exported_with_the_headers_signatures():
    from rgc_slam_amd import _lib
    protos = _header_protos()
    assert sorted(protos) == sorted(NAMES)
    assert len(protos["rgc_outlier_statistical"]) == 12 and len(protos["rgc_outlier_radius"]) == 12
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
            else:
                assert t is C.c_int, (name, p, t)
    hdr = open(os.path.join(ROOT, "include", "rgc_hip.h")).read()
    assert "#define RGC_OUTLIER_MAX_MEAN_K 63" in hdr and _lib.OUTLIER_MAX_MEAN_K == 63
    assert "[3P-memory]" in hdr[hdr.index("rgc_outlier_statistical --"):hdr.index("#define RGC_OUTLIER_MAX_MEAN_K")]


def test_the_info_structure_matches_the_compilers_layout(tmp_path):
    from rgc_slam_amd import _lib
    assert [n for n, _ in _lib.OutlierInfo._fields_] == FIELDS
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "rgc_hip.h"', "int main(void) {", '  printf("%zu", sizeof(rgc_outlier_info));']
    src += ['  printf(" %%zu", offsetof(rgc_outlier_info, %s));' % f for f in FIELDS] + ['  printf("\\n");', "  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    size, *offs = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()
    assert C.sizeof(_lib.OutlierInfo) == int(size) and [getattr(_lib.OutlierInfo, f).offset for f in FIELDS] == [int(o) for o in offs]


def test_null_arguments_are_invalid():
    from rgc_slam_amd import _lib
    L = _lib.load()
    kept = C.c_int(-7)
    info = _lib.OutlierInfo()
    assert L.rgc_outlier_statistical(None, None, 0, 12, 0, 8, 1.0, 0, None, None, None, C.byref(kept)) == _lib.ERR_INVALID and kept.value == -7
    assert L.rgc_outlier_radius(None, None, 0, 12, 0, 0.5, 2, 0, None, None, None, C.byref(kept)) == _lib.ERR_INVALID and kept.value == -7
    assert L.rgc_outlier_statistical(None, None, 0, 12, 0, 8, 1.0, 0, None, None, None, None) == _lib.ERR_INVALID
    assert L.rgc_outlier_radius(None, None, 0, 12, 0, 0.5, 2, 0, None, None, None, None) == _lib.ERR_INVALID
    assert L.rgc_outlier_get_info(None, C.byref(info)) == _lib.ERR_INVALID
    assert L.rgc_outlier_set_cell(None, 0.0) == _lib.ERR_INVALID


def test_the_python_mirror_imports_and_its_setters_refuse():
    import rgc_slam_amd
    from rgc_slam_amd import filters, odometry
    assert "filters" in rgc_slam_amd.__all__
    common = ("setInputCloud", "setNegative", "filter", "getIndices", "getRemovedIndices", "info")
    for name in common + ("setMeanK", "setStddevMulThresh"):
        assert callable(getattr(filters.StatisticalOutlierRemoval, name))
    for name in common + ("setRadiusSearch", "setMinNeighborsInRadius"):
        assert callable(getattr(filters.RadiusOutlierRemoval, name))
    assert callable(odometry.Preprocessor.statisticalOutlierRemoval) and callable(odometry.Preprocessor.radiusOutlierRemoval)
    # the setters check their ranges before any context exists (object.__new__: no device is opened here)
    s = object.__new__(filters.StatisticalOutlierRemoval)
    for bad in (0, -1, 64):
        with pytest.raises(filters.RgcError):
            s.setMeanK(bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(filters.RgcError):
            s.setStddevMulThresh(bad)
    s.setMeanK(63)
    s.setStddevMulThresh(-0.5)
    assert (s.getMeanK(), s.getStddevMulThresh()) == (63, -0.5)
    r = object.__new__(filters.RadiusOutlierRemoval)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e30):
        with pytest.raises(filters.RgcError):
            r.setRadiusSearch(bad)
    with pytest.raises(filters.RgcError):
        r.setMinNeighborsInRadius(-1)
    r.setRadiusSearch(0.5)
    r.setMinNeighborsInRadius(0)
    assert (r.getRadiusSearch(), r.getMinNeighborsInRadius()) == (0.5, 0)


def test_the_cpp_adaptors_compile_and_link(tmp_path):
    out = tmp_path / "test_filters"
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_filters.cpp"), "-o", str(out),
                           "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    assert out.exists()


def test_the_header_is_still_a_c99_header(tmp_path):
    src = tmp_path / "consumer.c"
    src.write_text('#include "rgc_hip.h"\nint main(void) { rgc_outlier_info s; s.n = RGC_OUTLIER_MAX_MEAN_K; return rgc_outlier_set_cell(0, 0.0) == RGC_ERR_INVALID && s.n == 63 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "consumer.o")])


def test_the_kernels_are_in_the_build_and_the_inventories_are_current():
    build = open(os.path.join(PKG, "build.py")).read()
    assert '"rgc_filters.hip"' in build and '"rgc_api_filters.hip"' in build
    for script in ("make_abi_index.py", "make_knobs.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--check"], capture_output=True, text=True)
        assert r.returncode == 0, (script, r.stdout, r.stderr)
