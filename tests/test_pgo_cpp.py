"""tests/cpp/test_pose_graph.cpp -- rgc::KeyframeStore::optimizePoseGraph and rgc::makeLoop of the C++ host layer -- compiles and links the way
tests/test_cpp_builds.py builds its programs (no GPU), and on the GPU prints the loop edge, the report and the corrected poses the Python class gives
for the same store."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")
SRC = os.path.join(ROOT, "tests", "cpp", "test_pose_graph.cpp")


def _build(out, flags):
    subprocess.check_call(["g++", "-std=c++14"] + flags + ["-pthread", SRC, "-o", str(out), "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    return str(out)


def test_the_pose_graph_program_compiles_and_links(tmp_path):
    assert os.path.exists(_build(tmp_path / "a.out", ["-O0", "-Wall", "-Wextra", "-Werror"]))


@pytest.mark.gpu
def test_cpp_pose_graph_matches_python(tmp_path):
    import pgo_cases as pc
    from rgc_slam_amd import keyframes, pose_graph
    exe = _build(tmp_path / "test_pose_graph", ["-O2", "-Wall"])
    poses = pc.trajectory(20, 321)
    with open(tmp_path / "poses.bin", "wb") as f:
        f.write(np.int32(len(poses)).tobytes()); f.write(poses.tobytes())
    r = subprocess.run([exe, str(tmp_path / "poses.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    ids = [10 + 2 * i for i in range(len(poses))]
    store = keyframes.KeyframeStore()
    try:
        for i, p in zip(ids, poses):
            store.push(i, p)
        T = np.eye(4, dtype=np.float32)
        T[:3, 3] = [0.3, -0.2, 0.05]
        graph = pose_graph.PoseGraph4DoF(store)
        e = graph.loop_from_icp(ids[-1], poses[-1], ids[1], poses[1], T)
        rep, out = store.optimize_pose_graph(ids, graph.loops, apply=True)
    finally:
        store.close()
    loop = [ln for ln in lines if ln.startswith("loop ")][0].split()[1:]
    assert [int(loop[0]), int(loop[1])] == [e.key_curr, e.key_loop]
    assert [float(v) for v in loop[2:]] == [*e.t_loop_curr[:], e.yaw_loop_curr_deg, e.pitch_loop_deg, e.roll_loop_deg]       # %.17g round-trips a double
    got = [ln for ln in lines if ln.startswith("report ")][0].split()[1:]
    mask = sum(1 << k for k, a in enumerate(rep["accepted"]) if a)
    assert [int(v) for v in got[:8]] == [rep["status"], rep["n_nodes"], rep["n_loops_used"], rep["fixed_id"], rep["iterations"], rep["successful"],
                                         pose_graph.STOP_NAMES.index(rep["stop"]), mask]
    assert [float(v) for v in got[8:]] == [rep["initial_cost"], rep["final_cost"]] and rep["successful"] >= 1
    cpp = np.array([[float(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("pose ")], np.float32)
    assert np.array_equal(cpp, out)                                                                                          # %.9g round-trips a float
    assert "no_loop 1" in r.stdout
