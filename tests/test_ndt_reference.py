"""NDT (P2D / D2D) without a GPU: the numpy reference tests/ndt_reference.py pinned to itself, and the new boundary -- every rgc_ndt_* symbol declared by
the header, exported by the library and bound by rgc_slam_amd/_lib.py (fails on a library without the feature), the struct mirror, the C++ mirror
compiling -Wall -Wextra -Werror.  The GPU side is tests/test_gpu_ndt.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ndt_reference as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")
NEW = ["rgc_default_ndt_params", "rgc_ndt_set_params", "rgc_ndt_get_params", "rgc_ndt_set_target", "rgc_ndt_set_source", "rgc_ndt_set_target_device",
       "rgc_ndt_set_source_device", "rgc_ndt_clear_source", "rgc_ndt_clear_target", "rgc_ndt_swap_source_and_target", "rgc_ndt_linearize",
       "rgc_ndt_compute_error", "rgc_ndt_num_correspondences", "rgc_ndt_align", "rgc_ndt_get_voxels", "rgc_ndt_get_raw_covariances"]


def _problem(seed, mode, method=nr.DIRECT7, radius=0.0, res=1.0, n=6000):
    rng = np.random.default_rng(seed)
    tgt = nr.scene(rng, n)
    T = nr.random_pose(rng, about=(100.0, -60.0, 2.0))
    src = (tgt[::3].astype(np.float64) @ np.linalg.inv(T)[:3, :3].T + np.linalg.inv(T)[:3, 3] + rng.normal(0, 0.01, (len(tgt[::3]), 3))).astype(np.float32)
    ndt = nr.NDT(res, mode, method, radius)
    ndt.set_target(tgt)
    ndt.set_source(src)
    return ndt, T


@pytest.mark.parametrize("mode", [nr.P2D, nr.D2D])
@pytest.mark.parametrize("method,radius", [(nr.DIRECT1, 0.0), (nr.DIRECT7, 0.0), (nr.DIRECT_RADIUS, 1.5)])
def test_b_is_half_the_gradient_of_the_frozen_cost(mode, method, radius):
    """The driver steps by d = -(H + lambda I)^-1 b and updates x <- [so3_exp(d[:3]) | d[3:]] * x (lsq_registration_impl.hpp:136-143).  Under that increment
    R a + t moves to first order by d[:3] x (R a + t) + d[3:], so e(d) = e + J d with J = [skew(R a + t), -I], and with the weights w and the matrices M
    frozen cost(d) = sum w (e + J d)^T M (e + J d): its gradient at d = 0 is +2 sum w J^T M e = +2 b.  The sign is the one that makes -H^-1 b the
    Gauss-Newton descent step.  Checked with central differences of step 1e-6 (truncation ~1e-12 relative, rounding ~1e-10 of the cost): 1e-6 relative
    to |b|."""
    ndt, T = _problem(81, mode, method, radius)
    y0, H, b = ndt.linearize(T)
    w = ndt.weights(T)
    assert ndt.num_terms() > 100
    h, g = 1e-6, np.zeros(6)
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        g[k] = (ndt.compute_error(nr.increment(d, T)[0], w) - ndt.compute_error(nr.increment(-d, T)[0], w)) / (2 * h)
    assert np.abs(g - 2 * b).max() <= 1e-6 * np.abs(b).max(), (g, 2 * b)
    assert np.array_equal(H, H.T) or np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
    assert np.linalg.eigvalsh(0.5 * (H + H.T)).min() >= -1e-9 * np.abs(H).max()
    assert ndt.compute_error(T) == pytest.approx(y0, rel=1e-14)


@pytest.mark.parametrize("r", [0.0, 1.0, 1.5, 2.0, 3.0])
def test_radius_offsets_against_brute_force(r):
    got = [tuple(o) for o in nr.offsets(nr.DIRECT_RADIUS, r)]
    m = int(np.ceil(r))
    brute = [(i, j, k) for i in range(-m, m + 1) for j in range(-m, m + 1) for k in range(-m, m + 1) if (i * i + j * j + k * k) ** 0.5 <= r + 1e-3]
    assert got == brute and len(set(got)) == len(got) and (0, 0, 0) in got
    assert len(got) == {0.0: 1, 1.0: 7, 1.5: 19, 2.0: 33, 3.0: 123}[r]
    assert len(nr.offsets(nr.DIRECT1)) == 1 and len(nr.offsets(nr.DIRECT7)) == 7 and len(nr.offsets(nr.DIRECT27)) == 27


def test_min_eig_clamps_below_and_leaves_alone_above():
    rng = np.random.default_rng(82)
    for _ in range(200):
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        w = 10.0 ** rng.uniform(-6, 1, 3)
        C = (Q * w) @ Q.T
        got = np.linalg.eigvalsh(nr.min_eig(C))
        want = np.sort(np.maximum(w, 1e-3))
        tol = 64 * np.finfo(np.float64).eps * want.max()      # a symmetric eigen-solve is backward stable: eigenvalues to a few eps |C|, here two solves and a product
        assert got.min() >= 1e-3 - tol
        assert np.abs(got - want).max() <= tol
        if w.min() >= 1e-3:
            assert np.abs(nr.min_eig(C) - C).max() <= 1e-14 * np.abs(C).max()
    assert np.abs(nr.min_eig(np.zeros((3, 3))) - 1e-3 * np.eye(3)).max() < 1e-18     # a voxel of one point, three equal eigenvalues


@pytest.mark.parametrize("mode", [nr.P2D, nr.D2D])
def test_the_gate_is_more_than_six_points(mode):
    rng = np.random.default_rng(83)
    six = (rng.uniform(0.6, 1.4, (6, 3)) + [10, 0, 0]).astype(np.float32)       # voxel (10, 0, 0) at res 1: six points
    seven = (rng.uniform(0.6, 1.4, (7, 3)) + [20, 0, 0]).astype(np.float32)     # voxel (20, 0, 0): seven
    ndt = nr.NDT(1.0, mode, nr.DIRECT1)
    ndt.set_target(np.concatenate([six, seven]))
    ndt.set_source(np.concatenate([six, seven]))
    ndt.linearize(np.eye(4))
    assert sorted(ndt.tmap.n.tolist()) == [6, 7]
    assert ndt.num_terms() == (7 if mode == nr.P2D else 1)
    assert set(ndt.tmap.n[ndt.corr[1]].tolist()) == {7}


def test_d2d_of_a_cloud_against_itself_has_no_gradient():
    rng = np.random.default_rng(84)
    cl = nr.scene(rng, 5000)
    ndt = nr.NDT(1.0, nr.D2D, nr.DIRECT1)
    ndt.set_target(cl)
    ndt.set_source(cl)
    cost, H, b = ndt.linearize(np.eye(4))
    assert ndt.num_terms() > 100 and cost == 0.0 and np.array_equal(b, np.zeros(6))


def test_the_wall_free_generator_regenerates_less_than_one_percent():
    """tests/test_gpu_ndt.py draws its clouds through ndt_reference.off_the_walls; the share it has to regenerate is asserted there and measured here with the
    reference alone (6 * 1e-4 * 2 per axis and resolution is the expected share: about 0.5 % over four resolutions and two poses)."""
    rng = np.random.default_rng(85)
    pts = nr.scene(rng, 20000)
    T = nr.random_pose(rng, about=(100.0, -60.0, 2.0))
    out, share = nr.off_the_walls(rng, pts, [np.eye(4), T], [0.5, 0.7, 1.0, 1.3], lambda k: nr.scene(rng, k))
    print("regenerated share: %.4f" % share)
    assert share < 0.01
    for res in (0.5, 0.7, 1.0, 1.3):
        assert nr.wall_distance(out.astype(np.float64), res).min() >= 1e-4


@pytest.fixture(scope="module")
def lib():
    from rgc_slam_amd import _lib
    return _lib


def test_the_new_entry_points_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "rgc_hip.h")).read()
    declared = sorted(set(re.findall(r"RGC_API[^;(]*?\b(rgc_(?:default_)?ndt_\w+)\s*\(", hdr)))
    assert declared == sorted(NEW)
    L = lib.load()
    for name in NEW:
        assert name in lib.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
    p = lib.NdtParams()
    L.rgc_default_ndt_params(C.byref(p))
    assert (p.resolution, p.distance_mode, p.neighbor_method, p.neighbor_radius) == (1.0, lib.NDT_D2D, lib.NDT_DIRECT7, 0.0)
    T = (C.c_double * 16)(*np.eye(4).ravel())
    g = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel())
    y, n = C.c_double(0), C.c_int(0)
    assert L.rgc_ndt_set_params(None, C.byref(p)) == -1 and L.rgc_ndt_get_params(None, C.byref(p)) == -1
    assert L.rgc_ndt_set_target(None, None, 0, 12) == -1 and L.rgc_ndt_set_source_device(None, None, 0, 12) == -1
    assert L.rgc_ndt_clear_source(None) == -1 and L.rgc_ndt_clear_target(None) == -1 and L.rgc_ndt_swap_source_and_target(None) == -1
    assert L.rgc_ndt_linearize(None, T, None, None, C.byref(y)) == -1 and L.rgc_ndt_compute_error(None, T, C.byref(y)) == -1
    assert L.rgc_ndt_num_correspondences(None, C.byref(n)) == -1 and L.rgc_ndt_align(None, g, None, None, None, None, None) == -1
    assert L.rgc_ndt_get_voxels(None, 0, 0, None, None, None, None, C.byref(n)) == -1 and L.rgc_ndt_get_raw_covariances(None, 0, 0, None, C.byref(n)) == -1


def test_struct_mirror_matches_the_header(lib, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rgc_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d\\n", sizeof(rgc_ndt_params), '
                   'offsetof(rgc_ndt_params, resolution), offsetof(rgc_ndt_params, distance_mode), offsetof(rgc_ndt_params, neighbor_method), '
                   'offsetof(rgc_ndt_params, neighbor_radius), RGC_NDT_MAX_OFFSETS); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    out = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(lib.NdtParams) and out[1:5] == [getattr(lib.NdtParams, f[0]).offset for f in lib.NdtParams._fields_]
    assert out[5] == lib.NDT_MAX_OFFSETS


def test_the_cpp_mirror_compiles_and_links(tmp_path):
    out = tmp_path / "test_ndt"
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_ndt.cpp"), "-o", str(out),
                           "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    assert out.exists()


def test_python_mirror_imports_without_a_gpu():
    from rgc_slam_amd import ndt
    assert ndt.NDTRegistration.setNeighborSearchMethod and ndt.NDT_DIRECT_RADIUS == 3
