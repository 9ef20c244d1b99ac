"""tests/cpp/test_keyframe_select.cpp -- rgc::KeyframeStore::travel / selectSurrounding / selectGlobal / detectLoop and rgc::uniformSampling of the C++
host layer -- compiles and links the way tests/test_cpp_builds.py builds its programs (no GPU), and on the GPU prints what the Python layer gives for the
same store."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")
SRC = os.path.join(ROOT, "tests", "cpp", "test_keyframe_select.cpp")


def _build(out, flags):
    subprocess.check_call(["g++", "-std=c++14"] + flags + ["-pthread", SRC, "-o", str(out), "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    return str(out)


def test_the_selection_program_compiles_and_links(tmp_path):
    assert os.path.exists(_build(tmp_path / "a.out", ["-O0", "-Wall", "-Wextra", "-Werror"]))


@pytest.mark.gpu
def test_cpp_selections_match_python(tmp_path):
    import us_cases as uc
    from rgc_slam_amd import keyframes, registration
    exe = _build(tmp_path / "test_keyframe_select", ["-O2", "-Wall"])
    poses, ids = uc.square_drive()
    with open(tmp_path / "poses.bin", "wb") as f:
        f.write(np.int32(len(poses)).tobytes()); f.write(poses.tobytes())
    r = subprocess.run([exe, str(tmp_path / "poses.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    pts = np.array([[0.1, 0.2, 0.3, 1], [-0.1, 0.2, 0, 2], [0.3, -0.2, 0.1, 3], [0, 0, 0.5, 4]], np.float32)
    store = keyframes.KeyframeStore()
    try:
        for i, p in zip(ids, poses):
            store.push(int(i), p, pts, pts[:2])
        d, a = store.travel(ids)
        assert [np.float32(v) for v in line["travel"]] == [d[-1], a[-1]]                          # %.9g round-trips a float
        sur, n_in = store.select_surrounding(poses[-1, :3], 15.0, 0.3, return_count=True)
        assert [int(v) for v in line["surrounding"]] == list(sur) and int(line["in_radius"][0]) == n_in and len(sur) > 10
        assert [int(v) for v in line["global"]] == list(store.select_global(0.5))
        det = store.detect_loop()
        assert [int(v) for v in line["loop"][:3]] == [1, det["latest_id"], det["closest_id"]] and det["found"] and det["closest_id"] == 10
        assert np.float32(line["loop"][3]) == np.float32(det["search_radius"]) and int(line["loop"][4]) == det["n_in_radius"]
        assert [int(v) for v in line["history"]] == list(det["history_ids"])
        d2 = store.detect_loop(min_key_id=0, history_search_num=2)
        assert [int(v) for v in line["loop2"]] == [int(d2["found"]), d2["closest_id"], len(d2["history_ids"])] and d2["closest_id"] == 7
    finally:
        store.close()
    _, idx = registration.uniform_sampling(np.ascontiguousarray(poses[:, :3]), 0.5, return_index=True)
    assert [int(v) for v in line["sampling"]] == list(idx)
