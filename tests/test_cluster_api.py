"""Euclidean cluster extraction's interface without a GPU: the rgc_cluster_* symbols are exported from the built library with the header's signatures, the
ctypes structure mirrors rgc_cluster_info field by field (names, sizeof and offsets against the C compiler), a NULL context or a NULL n_clusters is
RGC_ERR_INVALID, no crash and no output touched, segmentation.EuclideanClusterExtraction imports with PCL's member names and its setters refuse what the
C-ABI would, Preprocessor carries the member, the C++ adaptor compiles -Wall -Wextra -Werror against the header, the header is still a C99 header, both
new files are in the build, and the generated inventories are current."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")
NAMES = ["rgc_cluster_extract", "rgc_cluster_get_info", "rgc_cluster_set_cell"]
FIELDS = ["n", "n_components", "n_clusters", "n_clustered", "largest", "cell", "cells", "candidates"]


def _header_protos():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rgc_hip.h")).read(), flags=re.S)
    return {name: [a.strip() for a in args.split(",")] if args.strip() not in ("", "void") else []
            for name, args in re.findall(r"RGC_API\s+int\s+(rgc_cluster_\w+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)}


def test_the_symbols_are_exported_with_the_headers_signatures():
    from rgc_slam_amd import _lib
    protos = _header_protos()
    assert sorted(protos) == sorted(NAMES)
    assert len(protos["rgc_cluster_extract"]) == 12 and len(protos["rgc_cluster_get_info"]) == 2 and len(protos["rgc_cluster_set_cell"]) == 2
    L = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert getattr(raw, name) is not None and name in _lib.SYMBOLS
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
    block = hdr[hdr.index("rgc_cluster_extract --"):hdr.index("typedef struct rgc_cluster_info")]
    assert "[3P-memory]" in block and "do not call the PCL class" in hdr[hdr.index("Euclidean cluster extraction: pcl::"):hdr.index("rgc_cluster_extract --")]
    assert "ConditionalEuclideanClustering" in block and "indices-subset" in block              # the deviations are documented


def test_the_info_structure_matches_the_compilers_layout(tmp_path):
    from rgc_slam_amd import _lib
    assert [n for n, _ in _lib.ClusterInfo._fields_] == FIELDS
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "rgc_hip.h"', "int main(void) {", '  printf("%zu", sizeof(rgc_cluster_info));']
    src += ['  printf(" %%zu", offsetof(rgc_cluster_info, %s));' % f for f in FIELDS] + ['  printf("\\n");', "  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    size, *offs = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()
    assert C.sizeof(_lib.ClusterInfo) == int(size) and [getattr(_lib.ClusterInfo, f).offset for f in FIELDS] == [int(o) for o in offs]


def test_null_arguments_are_invalid_and_leave_the_outputs_alone():
    from rgc_slam_amd import _lib
    L = _lib.load()
    m = C.c_int(-7)
    info = _lib.ClusterInfo()
    cloud = np.zeros((4, 3), np.float32)
    out = [np.full(5, -77, np.int32) for _ in range(3)]
    ptrs = [o.ctypes.data for o in out]
    assert L.rgc_cluster_extract(None, cloud.ctypes.data, 4, 12, 0, 0.5, 1, 2 ** 31 - 1, *ptrs, C.byref(m)) == _lib.ERR_INVALID and m.value == -7
    assert L.rgc_cluster_extract(None, cloud.ctypes.data, 4, 12, 0, 0.5, 1, 2 ** 31 - 1, *ptrs, None) == _lib.ERR_INVALID
    assert L.rgc_cluster_extract(None, None, 0, 12, 0, 0.5, 1, 2 ** 31 - 1, None, None, None, None) == _lib.ERR_INVALID
    assert all((o == -77).all() for o in out)
    assert L.rgc_cluster_get_info(None, C.byref(info)) == _lib.ERR_INVALID
    assert L.rgc_cluster_set_cell(None, 0.0) == _lib.ERR_INVALID


def test_the_python_mirror_imports_and_its_setters_refuse():
    import rgc_slam_amd
    from rgc_slam_amd import odometry, segmentation
    assert "segmentation" in rgc_slam_amd.__all__
    for name in ("setInputCloud", "setClusterTolerance", "getClusterTolerance", "setMinClusterSize", "getMinClusterSize", "setMaxClusterSize", "getMaxClusterSize", "extract",
                 "labels", "info", "setCell"):
        assert callable(getattr(segmentation.EuclideanClusterExtraction, name)), name
    assert callable(odometry.Preprocessor.euclideanClusterExtraction)
    # the setters check their ranges before any context exists (object.__new__: no device is opened here)
    e = object.__new__(segmentation.EuclideanClusterExtraction)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e30):
        with pytest.raises(segmentation.RgcError):
            e.setClusterTolerance(bad)
    for bad in (0, -1):
        with pytest.raises(segmentation.RgcError):
            e.setMinClusterSize(bad)
        with pytest.raises(segmentation.RgcError):
            e.setMaxClusterSize(bad)
    e.setClusterTolerance(0.5)
    e.setMinClusterSize(1)
    e.setMaxClusterSize(2 ** 31 - 1)                 # PCL's defaults are accepted
    assert (e.getClusterTolerance(), e.getMinClusterSize(), e.getMaxClusterSize()) == (0.5, 1, 2 ** 31 - 1)
    e.setMinClusterSize(9)
    e.setMaxClusterSize(3)
    e._cloud = np.zeros((4, 3), np.float32)
    with pytest.raises(segmentation.RgcError):       # max_size < min_size: refused before any context is touched
        e.extract()


def test_the_cpp_adaptor_compiles_and_links(tmp_path):
    out = tmp_path / "test_segmentation"
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_segmentation.cpp"), "-o", str(out),
                           "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    assert out.exists()
    hpp = open(os.path.join(PKG, "cpp", "segmentation_hip.hpp")).read()
    for name in ("setInputCloud", "setClusterTolerance", "setMinClusterSize", "setMaxClusterSize", "getClusterTolerance", "getMinClusterSize", "getMaxClusterSize",
                 "void extract(std::vector<std::vector<int>>& clusters)", "int extract(int* d_labels, int* d_offsets, int* d_indices)"):
        assert name in hpp, name


def test_the_header_is_still_a_c99_header(tmp_path):
    src = tmp_path / "consumer.c"
    src.write_text('#include "rgc_hip.h"\nint main(void) { rgc_cluster_info s; int m = 0; s.n = 3; return rgc_cluster_set_cell(0, 0.0) == RGC_ERR_INVALID && '
                   'rgc_cluster_extract(0, 0, 0, 12, 0, 0.5, 1, 2147483647, 0, 0, 0, &m) == RGC_ERR_INVALID && s.n == 3 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "consumer.o")])


def test_both_files_are_in_the_build_and_the_inventories_are_current():
    build = open(os.path.join(PKG, "build.py")).read()
    assert '"rgc_cluster.hip"' in build and '"rgc_api_cluster.hip"' in build
    assert "RGC_LAB_CLUSTER_GROUP" in open(os.path.join(PKG, "csrc", "KNOBS.md")).read()
    for script in ("make_abi_index.py", "make_knobs.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--check"], capture_output=True, text=True)
        assert r.returncode == 0, (script, r.stdout, r.stderr)
