"""The boundary of FastGICPSingleThread without a GPU: every rgc_gicpst_* symbol declared by the header, exported by the library and bound by
rgc_slam_amd/_lib.py (fails on a library without the feature), a null context refused before HIP is touched, the Python mirror importable with the
method names of gicp.FastGICP plus reset / num_searched, the C++ mirror compiling -Wall -Wextra -Werror.  The GPU side is tests/test_gpu_gicp_st.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")
NEW = ["rgc_gicpst_reset", "rgc_gicpst_linearize", "rgc_gicpst_compute_error", "rgc_gicpst_num_correspondences", "rgc_gicpst_num_searched",
       "rgc_gicpst_get_correspondences", "rgc_gicpst_align"]


@pytest.fixture(scope="module")
def lib():
    from rgc_slam_amd import _lib
    return _lib


def test_the_new_entry_points_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "rgc_hip.h")).read()
    declared = sorted(set(re.findall(r"RGC_API[^;(]*?\b(rgc_gicpst_\w+)\s*\(", hdr)))
    assert declared == sorted(NEW)
    L = lib.load()
    for name in NEW:
        assert name in lib.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
    T = (C.c_double * 16)(*np.eye(4).ravel())
    g = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel())
    y, n = C.c_double(0), C.c_int(0)
    assert L.rgc_gicpst_reset(None) == -1
    assert L.rgc_gicpst_linearize(None, T, None, None, C.byref(y)) == -1 and L.rgc_gicpst_compute_error(None, T, C.byref(y)) == -1
    assert L.rgc_gicpst_num_correspondences(None, C.byref(n)) == -1 and L.rgc_gicpst_num_searched(None, C.byref(n)) == -1
    assert L.rgc_gicpst_get_correspondences(None, None, None, None, None) == -1
    assert L.rgc_gicpst_align(None, g, None, None, None, None, None, None) == -1


def test_the_python_mirror_has_fastgicps_names_and_its_own():
    from rgc_slam_amd import gicp
    st, base = gicp.FastGICPSingleThread, gicp.FastGICP
    assert issubclass(st, base)
    for name in ("linearize", "compute_error", "num_correspondences", "correspondences", "align"):
        assert getattr(st, name) is not getattr(base, name), name          # this method's, not FastGICP's
    for name in ("setMaxCorrespondenceDistance", "getMaxCorrespondenceDistance", "setInputTarget", "setInputSource", "setSourceCovariances"):
        assert getattr(st, name) is getattr(base, name), name
    assert callable(st.reset) and callable(st.num_searched)


def test_the_cpp_mirror_compiles_and_links(tmp_path):
    out = tmp_path / "test_gicp_st"
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_gicp_st.cpp"), "-o", str(out),
                           "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    assert out.exists()
    # the base class still compiles under the same flags with its members virtual
    out2 = tmp_path / "test_gicp"
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_gicp.cpp"), "-o", str(out2),
                           "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
