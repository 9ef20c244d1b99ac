"""FastGICPMultiPoints without a GPU: the numpy reference tests/gicp_mp_reference.py pinned to a literal restatement of fast_gicp_mp_impl.hpp:130-221 and to
itself (the Jacobian against central differences, a solve that recovers a pose), the designed cases of tests/gicp_mp_cases.py held to the minima they
declare, and the new boundary -- every entry point declared by the header, exported by the library and bound by rgc_slam_amd/_lib.py (fails on a library
without the feature), the struct's layout, the mirrors' method names, the C++ mirror compiling -Wall -Wextra -Werror.  The GPU side is
tests/test_gpu_gicp_mp.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gicp_mp_cases as mc
import gicp_mp_reference as mr
import gicp_reference as gr
import ndt_reference as nr
import nn_reference as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")
NEW = ["rgc_default_gicp_mp_params", "rgc_gicpmp_set_params", "rgc_gicpmp_get_params", "rgc_gicpmp_linearize", "rgc_gicpmp_num_correspondences",
       "rgc_gicpmp_num_candidates", "rgc_gicpmp_get_merged", "rgc_gicpmp_get_neighbors", "rgc_gicpmp_align"]
# the reference's public names (fast_gicp_mp.hpp:43-53), the pcl::Registration calls FastGICP has, the setter the reference forgot, and the read-outs
PY_METHODS = ["setNumThreads", "setRotationEpsilon", "setCorrespondenceRandomness", "setRegularizationMethod", "setInputSource", "setInputTarget",
              "setTransformationEpsilon", "setMaximumIterations", "getFinalTransformation", "hasConverged", "getFitnessScore", "setSourceCovariances",
              "setTargetCovariances", "clearSource", "clearTarget", "setNeighborSearchRadius", "linearize", "merged", "neighbors", "align"]
CPP_METHODS = ["setNumThreads", "setRotationEpsilon", "setCorrespondenceRandomness", "setRegularizationMethod", "setInputSource", "setInputTarget",
               "setTransformationEpsilon", "setMaximumIterations", "getFinalTransformation", "hasConverged", "getFitnessScore", "setSourceCovariances",
               "setTargetCovariances", "clearSource", "clearTarget", "setNeighborSearchRadius", "linearize", "merged", "neighbors", "align"]
CENTER = (100.0, -60.0, 2.0)


def _problem(seed, n=1500, k=10, r=0.5):
    rng = np.random.default_rng(seed)
    tgt = nr.scene(rng, n)
    T = nr.random_pose(rng, about=CENTER)
    Ti = np.linalg.inv(T)
    src = (tgt[::3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(0, 0.01, (len(tgt[::3]), 3))).astype(np.float32)
    g = mr.GICPMP(r)
    g.set_target(tgt, gr.knn_covariances(tgt, k))
    g.set_source(src, gr.knn_covariances(src, k))
    return g, T


@pytest.mark.parametrize("case", mc.all_cases(), ids=lambda c: c["name"])
def test_the_cases_hold_what_they_declare(case):
    cen = mc.census_of(case)
    print(case["name"], cen)
    short = {k: (cen[k], v) for k, v in case["minima"].items() if cen[k] < v}
    assert short == {}, short
    if "gate" in case:                                              # the dyadic cases: the gate is the lattice value the design assumes, every shell is there
        assert mr.r2_of(case["r"]) == np.float32(case["gate"] / 4096.0) and np.float32(case["gate"] / 4096.0) == case["gate"] / 4096.0
        keys = np.concatenate([np.concatenate([mc.rows_of(case["name"], p)["key"], mc.rows_of(case["name"], p)["out_key"]]) for p in range(len(case["poses"]))])
        members = np.concatenate([mc.rows_of(case["name"], p)["key"] for p in range(len(case["poses"]))])
        for units, least in case["key_counts"].items():
            assert int((keys == np.float32(units / 4096.0)).sum()) >= least, units
        assert not (members == np.float32(case["gate"] / 4096.0)).any()                              # the strict rule
        assert int((members == np.float32(case["shells"][0] / 4096.0)).sum()) >= case["key_counts"][case["shells"][0]]
    if case.get("whole"):
        for p in range(len(case["poses"])):
            assert (np.diff(mc.rows_of(case["name"], p)["off"]) == len(case["tgt"])).all()


def test_the_weight_is_the_reference_expression():
    """w = max(1e-3, min(1, 1 - sqrt(float key) / r)) with std::sqrt(float) (:184-185): the float32 root of numpy equals the rounded float64 root"""
    rng = np.random.default_rng(1)
    key = rng.uniform(0, 0.25, 100000).astype(np.float32)
    assert np.array_equal(np.sqrt(key), np.sqrt(key.astype(np.float64)).astype(np.float32))
    w, raw = mr.weights(np.float32([0.0, 1022 / 4096, 1021 / 4096, 0.25]), 0.5)
    assert w[0] == 1.0 and w[1] == 1e-3 and raw[1] < 1e-3 and w[2] == raw[2] > 1e-3 and w[3] == 1e-3
    assert abs(raw[1] - 0.00098) < 1e-5 and abs(raw[2] - 0.00147) < 1e-5


@pytest.mark.parametrize("r", [0.25, 0.5, 1.0])
def test_reference_equals_the_literal_restatement(r):
    """The vectorised 3x3 reference against the per-point 4x4 restatement (RCR(3,3) = 1, full inverse, 4-vectors): both add a row's members in ascending
    index, so they differ by the two inverses alone -- eps * cond(cov_B + R C_A R^T) <= 2.2e-16 * 2 / 2e-3 per entry of M, twice that for M M, summed with
    one sign: 1e-11 relative leaves more than an order of room."""
    g, T = _problem(21, n=1500, r=r)
    for P in (T, np.eye(4)):
        y, H, b = g.linearize(P)
        yl, Hl, bl, kept = mr.literal_linearize(g.source, g.cov_s, g.target, g.cov_t, P, r)
        assert kept == g.num_points() and kept > 50
        errs = (abs(y - yl) / abs(yl), np.abs(H - Hl).max() / np.abs(Hl).max(), np.abs(b - bl).max() / np.abs(bl).max())
        print("r %g: %d points, %d pairs, vectorised - literal %s" % (r, kept, g.num_pairs(), errs))
        assert max(errs) <= 1e-11
        yd, Hd, bd = g.linearize(P, descending=True, inverse=mr.adjugate_inverse)
        assert abs(yd - y) <= 1e-11 * abs(y) and np.abs(Hd - H).max() <= 1e-11 * np.abs(H).max()


def test_J_is_the_derivative_of_the_loss_under_the_drivers_update():
    """with the merge and M frozen, l(delta) = M (mean_B - (so3_exp(delta_r) (R p + t) + delta_t)), the loss after the driver's update
    T <- [so3_exp(delta_r) | delta_t] T: its derivative at 0 is J = M [skew(a) | -I].  Central differences, h = 1e-6: truncation h^2 |l'''| / 6 and
    rounding eps |l| / h are both below 1e-8 of the largest entry."""
    g, T = _problem(22, n=900)
    m = g.merge(T)
    i, l0, J, M = g.loss_rows(T, m)
    assert len(i) > 100
    h = 1e-6
    num = np.zeros_like(J)
    for a in range(6):
        d = np.zeros(6)
        d[a] = h
        lp = g.loss_rows(nr.increment(d, T)[0], m, M=M)[1]
        lm = g.loss_rows(nr.increment(-d, T)[0], m, M=M)[1]
        num[:, :, a] = (lp - lm) / (2 * h)
    assert np.abs(num - J).max() <= 1e-6 * np.abs(J).max(), np.abs(num - J).max() / np.abs(J).max()
    # ... and b = sum J^T l is half the gradient of the cost sum l.l, H = sum J^T J its Gauss-Newton matrix
    y, H, b = g.linearize(T)
    assert np.allclose(b, np.einsum("nia,ni->a", J, l0), rtol=1e-12, atol=1e-12 * np.abs(b).max())
    assert np.allclose(H, H.T, rtol=0, atol=1e-9 * np.abs(H).max()) and np.linalg.eigvalsh(H).min() > 0


def test_the_solve_recovers_the_pose():
    g, T = _problem(23, n=3000)
    X, iters, conv, failed, Hfin = g.align(np.eye(4))
    assert conv and not failed and 2 <= iters <= 64
    dT, d0 = X @ np.linalg.inv(T), np.linalg.inv(T)
    # the source carries 1 cm of noise per coordinate and is a third of a sparse map: the minimum lies within 3 sigma of the true pose, not on it
    assert np.abs(dT[:3, 3] - (np.eye(3) - dT[:3, :3]) @ np.array(CENTER)).max() < 0.03
    assert np.abs(dT[:3, :3] - np.eye(3)).max() < 0.25 * np.abs(d0[:3, :3] - np.eye(3)).max()
    far = np.eye(4)
    far[:3, 3] = [500.0, 500.0, 50.0]
    X, iters, conv, failed, _ = g.align(far)
    assert failed and not conv and iters == 1 and np.array_equal(X, far)        # no neighbour anywhere: failed at the guess


@pytest.fixture(scope="module")
def lib():
    from rgc_slam_amd import _lib
    return _lib


def test_the_new_entry_points_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "rgc_hip.h")).read()
    declared = sorted(set(re.findall(r"RGC_API[^;(]*?\b(rgc_gicpmp_\w+|rgc_default_gicp_mp_params)\s*\(", hdr)))
    assert declared == sorted(NEW)
    L = lib.load()
    for name in NEW:
        assert name in lib.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
    p = lib.GicpMpParams()
    L.rgc_default_gicp_mp_params(C.byref(p))
    assert (p.neighbor_search_radius, p.max_iterations, p.rotation_epsilon, p.transformation_epsilon) == (0.5, 64, 1e-5, 1e-5)
    L.rgc_default_gicp_mp_params(None)
    T = (C.c_double * 16)(*np.eye(4).ravel())
    g = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel())
    y, n, m = C.c_double(0), C.c_int(0), C.c_longlong(0)
    assert L.rgc_gicpmp_set_params(None, C.byref(p)) == -1 and L.rgc_gicpmp_get_params(None, C.byref(p)) == -1
    assert L.rgc_gicpmp_linearize(None, T, None, None, C.byref(y)) == -1
    assert L.rgc_gicpmp_num_correspondences(None, C.byref(n), C.byref(m)) == -1
    assert L.rgc_gicpmp_num_candidates(None, C.byref(m)) == -1
    assert L.rgc_gicpmp_get_merged(None, None, None, None, None) == -1
    assert L.rgc_gicpmp_get_neighbors(None, None, None, None, 0, C.byref(m)) == -1
    assert L.rgc_gicpmp_align(None, g, None, None, None, None, None, None) == -1


def test_the_struct_layout_matches_the_header(lib, tmp_path):
    """sizeof and every field's offset of _lib.GicpMpParams against the C compiler's view of rgc_gicp_mp_params (tests/test_abi.py's method)"""
    names = [f[0] for f in lib.GicpMpParams._fields_]
    assert names == ["neighbor_search_radius", "max_iterations", "rotation_epsilon", "transformation_epsilon"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "rgc_hip.h"', "int main(void) {", '  printf("%zu", sizeof(rgc_gicp_mp_params));']
    src += ['  printf(" %%zu", offsetof(rgc_gicp_mp_params, %s));' % n for n in names]
    src += ['  printf("\\n");', "  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    size, *offs = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()
    assert C.sizeof(lib.GicpMpParams) == int(size)
    assert [getattr(lib.GicpMpParams, n).offset for n in names] == [int(o) for o in offs]


def test_the_mirrors_carry_the_method_names():
    from rgc_slam_amd import gicp, registration
    assert issubclass(gicp.FastGICPMultiPoints, registration.FastVGICP)
    for m in PY_METHODS:
        assert callable(getattr(gicp.FastGICPMultiPoints, m)), m
    assert gicp.FastGICPMultiPoints.linearize is not registration.FastVGICP.linearize and gicp.FastGICPMultiPoints.align is not registration.FastVGICP.align
    assert gicp.FastGICPMultiPoints.setRotationEpsilon is not registration.FastVGICP.setRotationEpsilon
    hpp = open(os.path.join(PKG, "cpp", "fast_gicp_hip.hpp")).read()
    body = hpp[hpp.index("class FastGICPMultiPointsHip"):]
    base = re.match(r"class FastGICPMultiPointsHip\s*:\s*public\s+(\w+)", body)   # (its public base's members are its own: what it shares with FastGICPHip is declared once)
    if base:
        inherited = hpp[hpp.index("class %s {" % base.group(1)):]
        body += inherited[:inherited.index("\nprotected:")]
    for m in CPP_METHODS:
        assert re.search(r"\b%s\s*\(" % m, body), m


def test_the_cpp_mirror_compiles_and_links(tmp_path):
    out = tmp_path / "test_gicp_mp"
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_gicp_mp.cpp"), "-o", str(out),
                           "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    assert out.exists()
