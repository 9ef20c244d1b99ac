"""The 4-DoF pose graph without a GPU: the designed cases exercise what they declare (tests/pgo_cases.py, from the reference alone), the reference's
Jacobians are the derivatives of its residuals, rgc_pgo_make_loop (host only) against the reference's, the three structs against the C compiler,
bad arguments, and the two bars tests/test_gpu_pose_graph.py holds the kernels to -- measured here and printed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pgo_cases as pc
import pgo_reference as ref
from rgc_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_structural_minima_of_the_cases():
    cs = pc.cases()
    assert {cs[n]["sel_poses"].shape[0] for n in ("n1_no_loop", "n2_neighbours", "n3_fixed_middle")} == {1, 2, 3}
    fixed_places = set()
    for name, c in cs.items():
        g, e = pc.reference_graph(c), c["expect"]
        if e.get("refused"):
            assert g is None and len(c["loops"]) == 129, name
            continue
        assert g is not None, name
        assert g["status"] == e.get("status", ref.OPTIMIZED), name
        for key, have in (("fixed", g["fixed"]), ("n_used", len(g["used"])), ("n_ignored", g["n_ignored"])):
            if key in e:
                assert have == e[key], (name, key, have)
        N = g["N"]
        assert N <= 600
        if g["fixed"] >= 0:
            fixed_places.add("first" if g["fixed"] == 0 else "last" if g["fixed"] == N - 1 else "middle")
        loops = g["ij"][N - 1:]
        if e.get("neighbour_loop"):
            assert any(abs(int(a) - int(b)) == 1 for a, b in loops), name
        if e.get("loop_onto_fixed"):
            assert any(int(a) == g["fixed"] for a, b in loops), name
        if e.get("yaw_wrap"):     # the unnormalised rel_yaw of some odometry edge is beyond +-180, and some residual wraps at the perturbed state
            assert np.any(np.abs(g["meas"][:N - 1, 3]) > 180.0), name
            x = pc.perturbed(c)
            raw = x[g["ij"][:, 1], 0] - x[g["ij"][:, 0], 0] - g["meas"][:, 3]
            assert np.any(np.abs(raw) > 180.0), name
        # pitch and roll of several degrees, ids as declared
        assert N < 3 or np.abs(g["meas"][:, 4:6]).max() > 3.0, name
    assert fixed_places == {"first", "middle", "last"}
    assert cs["shared_node"]["ids"][1] - cs["shared_node"]["ids"][0] == 3                       # non-contiguous ids
    assert set(cs["ignored"]["ids"]) < set(cs["ignored"]["store_ids"])                              # a strict subset of the store
    g = pc.reference_graph(cs["nested_crossing"])
    a = [tuple(sorted(map(int, p))) for p in g["ij"][g["N"] - 1:]]
    assert any(p[0] < q[0] and q[1] < p[1] for p in a for q in a) and any(p[0] < q[0] < p[1] < q[1] for p in a for q in a)   # nested, crossing
    g = pc.reference_graph(cs["shared_node"])
    ends = [int(v) for p in g["ij"][g["N"] - 1:] for v in p]
    assert len(set(ends)) < len(ends)
    g = pc.reference_graph(cs["big_100_on_300"])
    assert g["N"] == 300 and len(g["used"]) == 100
    assert [pc.reference_graph(cs[n])["N"] for n in ("seg_S-1", "seg_S", "seg_S+1", "seg_2S+1")] == [pc.SEGMENT - 1, pc.SEGMENT, pc.SEGMENT + 1, 2 * pc.SEGMENT + 1]


@pytest.mark.parametrize("name", pc.SOLVE_CASES)
def test_lm_path_minima_of_the_cases(name):
    g, x0, x, info = pc.reference_solve(name)
    e = pc.cases()[name]["expect"]
    pc.check_margins(info)
    if "stop" in e:
        assert info["stop"] == e["stop"], info
    if "iterations" in e:
        assert info["iterations"] == e["iterations"]
    rejected = sum(1 for s in info["steps"] if not s["accepted"])
    assert rejected >= e.get("min_rejected", 0) and info["successful"] >= e.get("min_accepted", 1), info
    assert info["final_cost"] < info["initial_cost"]
    # loop errors of decimetres and degrees: macroscopic residuals
    assert info["initial_cost"] > 1e-2
    # the reference's round trip through degrees returns the stored pitch and roll
    c = pc.cases()[name]
    _, pitch, roll = ref.state_of(c["sel_poses"])
    assert np.array_equal((pitch * ref.DEG2RAD).astype(np.float32), c["sel_poses"][:, 4]) and np.array_equal((roll * ref.DEG2RAD).astype(np.float32), c["sel_poses"][:, 3])


def test_reference_jacobians_are_the_derivatives_of_its_residuals():
    c = pc.cases()["nested_crossing"]
    g = pc.reference_graph(c)
    x = pc.perturbed(c).astype(ref.LD)
    _, Ji, Jj = ref.edge_terms(g["ij"], g["meas"], x, -1)
    h = ref.LD(1e-9)
    for e in (0, 17, g["N"] - 1, len(g["ij"]) - 1):
        i, j = map(int, g["ij"][e])
        for node, J in ((i, Ji), (j, Jj)):
            for k in range(4):
                xp, xm = x.copy(), x.copy()
                xp[node, k] += h
                xm[node, k] -= h
                rp = ref.edge_terms(g["ij"][e:e + 1], g["meas"][e:e + 1], xp, -1)[0][0]
                rm = ref.edge_terms(g["ij"][e:e + 1], g["meas"][e:e + 1], xm, -1)[0][0]
                assert np.allclose(((rp - rm) / (2 * h)).astype(np.float64), J[e][:, k].astype(np.float64), atol=1e-7), (e, node, k)


def _lib_make_loop(latest, loop, T, kc, kl):
    from rgc_slam_amd import pose_graph
    return pose_graph.make_loop(latest, loop, T, kc, kl)


def test_make_loop_against_the_reference():
    rng = np.random.default_rng(77)
    for trial in range(20):
        poses = pc.trajectory(30, 100 + trial, turn_deg=9.0)
        latest, loop = poses[29], poses[int(rng.integers(0, 20))]
        ang = np.deg2rad(rng.normal(0, 3.0))
        T = np.eye(4, dtype=np.float32)
        T[:2, :2] = [[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]
        T[:3, 3] = rng.normal(0, 0.4, 3)
        got = _lib_make_loop(latest, loop, T, 29, 4)
        f32, f64 = ref.make_loop(latest, loop, T, 29, 4, np.float32), ref.make_loop(latest, loop, T, 29, 4, np.float64)
        assert (got.key_curr, got.key_loop) == (29, 4)
        assert got.pitch_loop_deg == f32["pitch"] and got.roll_loop_deg == f32["roll"]
        # fp32 products of three affine matrices whose entries are below `reach`: a dozen roundings of 2^-24 each on the translation, as many on a
        # rotation entry of magnitude <= 1; the fp32 reference agrees with the library to that, and both with exact arithmetic
        reach = float(np.abs(poses[:, :3]).max()) + 1.0
        tol_t, tol_yaw = 24 * 2.0 ** -24 * reach, 24 * 2.0 ** -24 * ref.RAD2DEG
        for want in (f32, f64):
            assert np.abs(np.array(got.t_loop_curr[:]) - want["t"]).max() <= tol_t, (trial, got.t_loop_curr[:], want["t"])
            assert abs(ref.normalize_angle(got.yaw_loop_curr_deg - want["yaw"])) <= tol_yaw, (trial, got.yaw_loop_curr_deg, want["yaw"])
    L = _lib.load()
    out = _lib.PgoLoop()
    p = _lib.KfPose(0, 0, 0, 0, 0, 0)
    T = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel())
    assert L.rgc_pgo_make_loop(None, C.byref(p), T, 1, 0, C.byref(out)) == _lib.ERR_INVALID
    assert L.rgc_pgo_make_loop(C.byref(p), C.byref(p), None, 1, 0, C.byref(out)) == _lib.ERR_INVALID
    assert L.rgc_pgo_make_loop(C.byref(p), C.byref(p), T, 1, 0, None) == _lib.ERR_INVALID
    T[3] = float("nan")
    assert L.rgc_pgo_make_loop(C.byref(p), C.byref(p), T, 1, 0, C.byref(out)) == _lib.ERR_INVALID


def test_null_arguments_are_invalid_without_a_gpu():
    L = _lib.load()
    rep = _lib.PgoReport()
    ids = (C.c_int * 2)(0, 1)
    assert L.rgc_pgo_optimize(None, ids, 2, None, 0, None, 0, None, C.byref(rep)) == _lib.ERR_INVALID
    assert L.rgc_pgo_linearize(None, ids, 2, None, 0, None, 0.0, None, None, None, None, None, None, None, None, None, C.byref(rep)) == _lib.ERR_INVALID
    L.rgc_default_pgo_params(None)
    prm = _lib.PgoParams()
    L.rgc_default_pgo_params(C.byref(prm))
    assert (prm.max_iterations, prm.initial_radius) == (10, 1e4)


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof and every field's offset of the three ctypes mirrors against the C compiler's view of include/rgc_hip.h (the method of
    tests/test_abi.py::test_python_mirror_struct_layouts_match_the_header)"""
    pairs = {"rgc_pgo_loop": _lib.PgoLoop, "rgc_pgo_params": _lib.PgoParams, "rgc_pgo_report": _lib.PgoReport}
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgc_hip.h")).read(), flags=re.S)
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "rgc_hip.h"', "int main(void) {"]
    found = {}
    for m in re.finditer(r"typedef struct (rgc_\w+)\s*\{(.*?)\}\s*\1\s*;", h, re.S):
        if m.group(1) not in pairs:
            continue
        names = []
        for decl in m.group(2).split(";"):
            if decl.strip():
                for part in decl.strip().split(","):
                    names.append(re.sub(r"\[.*", "", part.strip().split()[-1].lstrip("*")))
        found[m.group(1)] = names
        src.append(f'  printf("{m.group(1)} %zu", sizeof({m.group(1)}));')
        src += [f'  printf(" %zu", offsetof({m.group(1)}, {n}));' for n in names]
        src.append('  printf("\\n");')
    src += ["  return 0;", "}"]
    assert set(found) == set(pairs)
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    out = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == 3
    for line in out:
        s, size, *offs = line.split()
        cls = pairs[s]
        assert C.sizeof(cls) == int(size), (s, C.sizeof(cls), size)
        assert [f[0] for f in cls._fields_] == found[s], s
        assert [getattr(cls, f[0]).offset for f in cls._fields_] == [int(o) for o in offs], s


def test_the_two_bars_are_measured_and_printed():
    term, step = pc._fp64_deviations()
    for n in pc.TERM_CASES:
        print("pose graph fp64 deviation  %-24s terms %.2e  step %.2e" % (n, term[n], step[n]))
    tb, sb, tm, sm = pc.term_bar(), pc.step_bar(), pc.term_bar("one_loop"), pc.step_bar("one_loop")
    print("pose graph bars: all cases: terms %.3e step %.3e; metre-scale cases: terms %.3e step %.3e" % (tb, sb, tm, sm))
    # a plain fp64 evaluation is a few roundings off; a bar far above that would check nothing
    assert 0 < tm <= tb < 1e-10 and 0 < sm <= sb < 1e-8 and tm < 1e-12 and sm < 1e-11
