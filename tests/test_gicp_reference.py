"""FastGICP without a GPU: the numpy reference tests/gicp_reference.py pinned to a literal restatement of fast_gicp_impl.hpp:115-211 and to itself
(gradient, self-registration, the strict gate), and the new boundary -- every rgc_gicp_* symbol declared by the header, exported by the library and bound
by rgc_slam_amd/_lib.py (fails on a library without the feature), the Python mirror importable, the C++ mirror compiling -Wall -Wextra -Werror.  The GPU
side is tests/test_gpu_gicp.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gicp_reference as gr
import ndt_reference as nr
import nn_reference as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")
NEW = ["rgc_gicp_set_max_correspondence_distance", "rgc_gicp_get_max_correspondence_distance", "rgc_gicp_linearize", "rgc_gicp_compute_error",
       "rgc_gicp_num_correspondences", "rgc_gicp_get_correspondences", "rgc_gicp_align"]
CENTER = (100.0, -60.0, 2.0)


def _problem(seed, n=1500, k=10, d_max=gr.FLT_MAX):
    rng = np.random.default_rng(seed)
    tgt = nr.scene(rng, n)
    T = nr.random_pose(rng, about=CENTER)
    Ti = np.linalg.inv(T)
    src = (tgt[::3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(0, 0.01, (len(tgt[::3]), 3))).astype(np.float32)
    g = gr.GICP(d_max)
    g.set_target(tgt, gr.knn_covariances(tgt, k))
    g.set_source(src, gr.knn_covariances(src, k))
    return g, T


@pytest.mark.parametrize("d_max", [gr.FLT_MAX, 0.5])
def test_reference_equals_the_literal_restatement(d_max):
    """The vectorised 3x3 reference against the per-point 4x4 restatement (RCR(3,3) = 1, full inverse, M(3,3) = 0): the two differ by the rounding of the
    two inverses -- eps * cond(C_B + R C_A R^T) <= eps * 2 / 2e-3 per matrix entry, so 1e-11 relative on the sums leaves two orders of room."""
    g, T = _problem(11, n=1500, d_max=d_max)
    for P in (T, np.eye(4)):
        y, H, b = g.linearize(P)
        yl, Hl, bl = gr.literal_linearize(g.source, g.cov_s, g.target, g.cov_t, P, d_max)
        assert g.num_kept() > 10
        assert abs(y - yl) <= 1e-11 * abs(yl)
        assert np.abs(H - Hl).max() <= 1e-11 * np.abs(Hl).max() and np.abs(b - bl).max() <= 1e-11 * np.abs(bl).max()
    if d_max < 1.0:
        g.linearize(np.eye(4))
        assert 0 < g.num_kept() < len(g.source)        # the gate rejects some at the unaligned pose


def test_b_is_half_the_gradient_of_the_frozen_cost():
    g, T = _problem(12)
    _, H, b = g.linearize(T)
    h = 1e-6
    grad = np.zeros(6)
    for a in range(6):
        d = np.zeros(6)
        d[a] = h
        grad[a] = (g.compute_error(nr.increment(d, T)[0]) - g.compute_error(nr.increment(-d, T)[0])) / (2 * h)
    # central differences: truncation h^2 |f'''| / 6 and rounding eps |f| / h, both far below 1e-5 of the gradient's largest entry here
    assert np.abs(0.5 * grad - b).max() <= 1e-5 * np.abs(b).max(), (grad, b)
    assert np.allclose(H, H.T, rtol=0, atol=1e-9 * np.abs(H).max()) and np.linalg.eigvalsh(H).min() > 0


def test_self_registration_costs_nothing():
    rng = np.random.default_rng(13)
    P = nr.scene(rng, 900)
    cov = gr.knn_covariances(P, 10)
    g = gr.GICP()
    g.set_target(P, cov)
    g.set_source(P, cov)
    y, H, b = g.linearize(np.eye(4))
    idx, key = g.corr[0], g.corr[1]
    assert np.array_equal(idx, np.arange(len(P))) and not key.any()
    assert y == 0.0 and not b.any() and np.abs(H).max() > 0
    assert g.compute_error(np.eye(4)) == 0.0


def test_the_gate_is_strict():
    """lattice points exactly ON the gate (squared distance == d_max^2: rejected) and one lattice unit inside it (kept); every key is exact"""
    It = np.array([[0, 0, 0], [640, 0, 0], [0, 640, 0], [640, 640, 64]])
    gate_units = 32                                                                   # 0.5 m
    Iq = np.array([[gate_units, 0, 0], [640 + gate_units - 1, 0, 0], [0, 640 - gate_units, 0], [640, 640, 64 + gate_units - 1], [640, 640 + gate_units, 64]])
    tgt, src = nn.lattice(It), nn.lattice(Iq)
    eye = np.broadcast_to(np.eye(3), (len(tgt), 3, 3))
    g = gr.GICP(d_max=gate_units * nn.STEP)
    g.set_target(tgt, eye)
    g.set_source(src, np.broadcast_to(np.eye(3), (len(src), 3, 3)))
    idx, key = g.correspondences(np.eye(4))
    assert np.array_equal(key, np.float32([0.25, (31 / 64) ** 2, 0.25, (31 / 64) ** 2, 0.25]))
    assert idx.tolist() == [-1, 1, -1, 3, -1]
    y, H, b = g.linearize(np.eye(4))
    assert g.num_kept() == 2 and y == pytest.approx(2 * 0.5 * (31 / 64) ** 2, rel=1e-15)  # M = (I + I)^-1
    g.d_max = np.nextafter(gate_units * nn.STEP, 1.0)
    assert g.correspondences(np.eye(4))[0].tolist() == [0, 1, 2, 3, 3]
    g.d_max = 0.0
    assert g.linearize(np.eye(4))[0] == 0.0 and g.num_kept() == 0 and not g.linearize(np.eye(4))[1].any()


def test_the_solve_recovers_the_pose():
    g, T = _problem(14, n=3000)
    X, iters, conv, failed, Hfin = g.align(np.eye(4))
    assert conv and not failed and 2 <= iters <= 30
    dT, d0 = X @ np.linalg.inv(T), np.linalg.inv(T)
    # the source carries 1 cm of noise per coordinate and is a third of a sparse map: the minimum lies within 3 sigma of the true pose, not on it
    assert np.abs(dT[:3, 3]).max() < 0.03 and np.abs(dT[:3, 3]).max() < 0.25 * np.abs(d0[:3, 3] - (np.eye(3) - d0[:3, :3]) @ np.array(CENTER)).max()
    assert np.abs(dT[:3, :3] - np.eye(3)).max() < 0.25 * np.abs(d0[:3, :3] - np.eye(3)).max()
    assert np.array_equal(Hfin, Hfin.T) or np.allclose(Hfin, Hfin.T)


@pytest.fixture(scope="module")
def lib():
    from rgc_slam_amd import _lib
    return _lib


def test_the_new_entry_points_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "rgc_hip.h")).read()
    declared = sorted(set(re.findall(r"RGC_API[^;(]*?\b(rgc_gicp_\w+)\s*\(", hdr)))
    assert declared == sorted(NEW)
    L = lib.load()
    for name in NEW:
        assert name in lib.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
    T = (C.c_double * 16)(*np.eye(4).ravel())
    g = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel())
    y, n = C.c_double(0), C.c_int(0)
    assert L.rgc_gicp_set_max_correspondence_distance(None, 1.0) == -1 and L.rgc_gicp_get_max_correspondence_distance(None, C.byref(y)) == -1
    assert L.rgc_gicp_linearize(None, T, None, None, C.byref(y)) == -1 and L.rgc_gicp_compute_error(None, T, C.byref(y)) == -1
    assert L.rgc_gicp_num_correspondences(None, C.byref(n)) == -1 and L.rgc_gicp_get_correspondences(None, None, None) == -1
    assert L.rgc_gicp_align(None, g, None, None, None, None, None, None) == -1


def test_the_cpp_mirror_compiles_and_links(tmp_path):
    out = tmp_path / "test_gicp"
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_gicp.cpp"), "-o", str(out),
                           "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    assert out.exists()


def test_python_mirror_imports_without_a_gpu():
    from rgc_slam_amd import gicp, registration
    assert issubclass(gicp.FastGICP, registration.FastVGICP)
    for m in ("setInputSource", "setInputTarget", "setCorrespondenceRandomness", "setRegularizationMethod", "setMaxCorrespondenceDistance", "setSourceCovariances",
              "setTargetCovariances", "swapSourceAndTarget", "clearSource", "clearTarget", "linearize", "compute_error", "align", "correspondences"):
        assert callable(getattr(gicp.FastGICP, m)), m
    assert gicp.FastGICP.linearize is not registration.FastVGICP.linearize and gicp.FastGICP.align is not registration.FastVGICP.align
