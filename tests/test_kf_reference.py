"""The keyframe store (f5) without a GPU: the independent reference tests/kf_reference.py against scipy, the new entry points exported and refusing a
NULL context before they touch HIP, the ctypes mirrors of the two new structs, and the C++ mirror (rgc-slam_amd/cpp/keyframe_store.hpp) compiling
-Wall -Wextra -Werror.  The GPU side is tests/test_gpu_keyframes.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kf_reference as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")
NEW = ["rgc_kf_reset", "rgc_kf_push", "rgc_kf_set_poses", "rgc_kf_get_info", "rgc_kf_assemble", "rgc_mapreg_set_maps_device", "rgc_icp_align_device"]


def _scipy_matrix(pose):
    from scipy.spatial.transform import Rotation
    p = kr.pose_f32(pose).astype(np.float64)
    return Rotation.from_euler("ZYX", [p[5], p[4], p[3]]).as_matrix()     # intrinsic z-y'-x'' = Rz(yaw) Ry(pitch) Rx(roll)


def test_rotation_matches_scipy_on_drawn_poses():
    seed = 7101
    rng = np.random.default_rng(seed)
    worst = 0.0
    for _ in range(2000):
        pose = np.concatenate([rng.uniform(-2000, 2000, 3), [rng.uniform(-np.pi, np.pi), rng.uniform(-np.pi / 2, np.pi / 2), rng.uniform(-np.pi, np.pi)]])
        d = float(np.abs(kr.rotation(pose).astype(np.float64) - _scipy_matrix(pose)).max())
        worst = max(worst, d)
        assert d <= 1e-15, (seed, pose, d)
    print("largest element difference to scipy: %.3g" % worst)


def test_rotation_matches_scipy_next_to_the_gimbal_lock():
    seed = 7102
    rng = np.random.default_rng(seed)
    for _ in range(2000):
        pitch = rng.choice([-1.0, 1.0]) * (np.pi / 2 - rng.uniform(0, 1e-3))
        pose = np.array([0, 0, 0, rng.uniform(-np.pi, np.pi), pitch, rng.uniform(-np.pi, np.pi)])
        d = float(np.abs(kr.rotation(pose).astype(np.float64) - _scipy_matrix(pose)).max())
        assert d <= 1e-15, (seed, pose, d)
        R = kr.rotation(pose)
        assert float(np.abs(R @ R.T - np.eye(3)).max()) < 1e-17 * 100      # a rotation, to the longdouble's precision


def test_concatenation_order_and_empty_kinds():
    rng = np.random.default_rng(7103)
    mk = lambda n: rng.normal(0, 10, (n, 4)).astype(np.float32)
    clouds = {5: [mk(3), mk(0), mk(2)], 9: [mk(0), mk(4), mk(1)], 2: [mk(1), mk(1), mk(0)]}
    poses = {i: np.array([i, -i, 0.5, 0.1, -0.2, 0.3 * i]) for i in clouds}
    a = kr.assemble(clouds, poses, [9, 5, 9, 2], 0b011)
    assert [(i, k, n) for i, k, _, n in a.segments] == [(9, 1, 4), (5, 0, 3), (9, 1, 4), (2, 0, 1), (2, 1, 1)]
    assert a.n == 13 and np.array_equal(a.c[:4], clouds[9][1][:, 3]) and np.array_equal(a.c[4:7], clouds[5][0][:, 3])
    assert np.array_equal(a.xyz[0:4], a.xyz[7:11])                      # a repeated id: the same points again
    assert kr.assemble(clouds, poses, [], 0b111).n == 0 and kr.assemble(clouds, poses, [9], 0b001).n == 0
    # the identity pose leaves a cloud where it is
    assert np.array_equal(kr.transform_cloud(clouds[5][0], np.zeros(6)).astype(np.float32), clouds[5][0][:, :3])


@pytest.fixture(scope="module")
def lib():
    from rgc_slam_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("rgc_build", os.path.join(PKG, "build.py"))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
        m.build()
    return _lib


def test_the_new_entry_points_are_exported_and_refuse_a_null_context(lib):
    """(this is the test that fails on the parent commit: it has none of these symbols)"""
    hdr = open(os.path.join(ROOT, "include", "rgc_hip.h")).read()
    raw = C.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert ("RGC_API int %s(" % name) in hdr, name
        assert name in lib.SYMBOLS, name
        assert hasattr(raw, name), name
    L = lib.load()
    pose, info, n = lib.KfPose(), lib.KfInfo(), (C.c_int * 2)()
    pts = np.zeros((8, 4), np.float32)
    ids = (C.c_int * 1)(0)
    prm, res, T = lib.IcpParams(), lib.IcpResult(), np.zeros(16, np.float32)
    L.rgc_default_icp_params(C.byref(prm))
    fp = C.POINTER(C.c_float)
    assert L.rgc_kf_reset(None) == lib.ERR_INVALID
    assert L.rgc_kf_push(None, 0, C.byref(pose), pts.ctypes.data, 8, pts.ctypes.data, 8, pts.ctypes.data, 8, 16, 0) == lib.ERR_INVALID
    assert L.rgc_kf_set_poses(None, ids, C.byref(pose), 1) == lib.ERR_INVALID
    assert L.rgc_kf_get_info(None, C.byref(info)) == lib.ERR_INVALID
    assert L.rgc_kf_assemble(None, ids, 1, 3, 0.0, pts.ctypes.data, 8, 0, n, C.cast(C.byref(n, 4), C.POINTER(C.c_int))) == lib.ERR_INVALID
    assert L.rgc_mapreg_set_maps_device(None, pts.ctypes.data, 8, pts.ctypes.data, 8, 16) == lib.ERR_INVALID
    assert L.rgc_icp_align_device(None, pts.ctypes.data, 8, pts.ctypes.data, 8, 16, C.byref(prm), T.ctypes.data_as(fp), C.byref(res)) == lib.ERR_INVALID
    assert (lib.KF_CORNER, lib.KF_SURF, lib.KF_SCAN, lib.KF_KINDS) == (0, 1, 2, 3)


def test_struct_mirrors_match_the_header(lib, tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "rgc_hip.h"', "int main(void) {",
           '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rgc_kf_pose), offsetof(rgc_kf_pose, x), offsetof(rgc_kf_pose, y), offsetof(rgc_kf_pose, z), offsetof(rgc_kf_pose, roll), offsetof(rgc_kf_pose, pitch), offsetof(rgc_kf_pose, yaw));',
           '  printf("%zu %zu %zu %zu\\n", sizeof(rgc_kf_info), offsetof(rgc_kf_info, n_keyframes), offsetof(rgc_kf_info, n_points), offsetof(rgc_kf_info, revision));',
           '  printf("%d %d %d %d\\n", RGC_KF_CORNER, RGC_KF_SURF, RGC_KF_SCAN, RGC_KF_KINDS);', "  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    out = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, cls in zip(out[:2], (lib.KfPose, lib.KfInfo)):
        size, *offs = [int(v) for v in line.split()]
        assert C.sizeof(cls) == size and [getattr(cls, f[0]).offset for f in cls._fields_] == offs, (cls, line)
    assert out[2].split() == ["0", "1", "2", "3"]


def test_the_cpp_mirror_compiles_and_links(tmp_path):
    out = tmp_path / "a.out"
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_keyframe_store.cpp"), "-o", str(out),
                           "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    assert out.exists()


def test_python_mirror_imports_without_a_gpu():
    from rgc_slam_amd import keyframes
    assert keyframes.KeyframeStore.kind_mask((keyframes.KF_CORNER, keyframes.KF_SURF)) == 3 and keyframes.KeyframeStore.kind_mask(keyframes.KF_SCAN) == 4
