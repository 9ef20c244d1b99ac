"""The CPU oracle's voxel stage against tests/vgicp_reference.py (numpy only) at any voxel size and every neighbour search method.

Before, every test and campaign drew the resolution from {0.5, 1, 2}: powers of two, where x / res and x * (1 / res) are the same double,
and only the oracle's own restatement (oracle/py_oracle.py) looked at DIRECT7 / DIRECT27.  Here, with the oracle's per-point covariances
as the input (so the k-NN stage is not under test), at resolutions {0.3, 0.5, 0.75, 1.0, 1.7, 3.0}, DIRECT1 / 7 / 27, the three
accumulation modes and PLANE / MIN_EIG covariances, on the synthetic map and scan, a copy 1e4 m from the origin and points on voxel walls:

  * voxel coordinates, counts, order and correspondence counts exactly; means 1e-12 relative (MULTIPLICATIVE: two 4x4 inversions,
    1e-9); covariances, H, b and cost 1e-9 relative;
  * ADDITIVE and ADDITIVE_WEIGHTED give the same voxel table, bit for bit, and the same linearisation.

No GPU; about 20 s."""
import numpy as np
import pytest

import vgicp_reference as vr

RES = [0.3, 0.5, 0.75, 1.0, 1.7, 3.0]
WALL_CELLS = [-9, -4, -1, 0, 2, 7, 12, 22, 27]
FAR = np.float32([1.0e4, -1.0e4, 3.0e3])


def _pose(yaw, pitch, roll, t):
    import rgc_slam_amd.synth as synth
    return synth.se3(synth.rot_zyx(yaw, pitch, roll), t)


@pytest.fixture(scope="module")
def clouds():
    import rgc_slam_amd.synth as synth
    world, tgt = synth.make_world_and_map(4000, seed=synth.SEED + 51)
    T_true = _pose(0.015, 0.003, -0.002, [0.12, 0.04, 0.01])
    src = synth.make_scan_n(world, T_true, 1500, seed=synth.SEED + 51)["xyz"]
    return dict(synthetic=(tgt, src), far=(tgt + FAR, src + FAR), walls=_walls(1.0))


def _walls(res, seed=5):
    """a target of wall values on every axis (each coordinate on or next to a wall) and a source of the same kind"""
    rng = np.random.default_rng(seed)
    v = vr.wall_values(res, WALL_CELLS)
    tgt = rng.choice(v, (2000, 3)).astype(np.float32)
    src = rng.choice(v, (800, 3)).astype(np.float32)
    return tgt, src


def _oracle(orc, tgt, src, res, method, mode, reg):
    o = orc.Registration(voxel_res=res, neighbor_method=vr.METHODS.index(method), voxel_mode=vr.MODES.index(mode), regularization=reg,
                         num_threads=0)
    o.set_target(tgt); o.set_source(src); o.prepare()
    return o


def _check_table(got, ref, what, mean_bar):
    got = vr.in_cell_order(got)
    assert np.array_equal(got["coords"], ref["coords"]), f"{what}: voxel coordinates / order differ ({len(got['coords'])} vs {len(ref['coords'])})"
    assert np.array_equal(got["num"], ref["num"]), f"{what}: voxel counts"
    e = np.abs(got["mean"] - ref["mean"]).max(axis=1) / np.maximum(np.abs(ref["mean"]).max(axis=1), 1e-300)
    assert e.max() <= mean_bar, f"{what}: means {e.max():.2e}"
    e = np.abs(got["cov"] - ref["cov"]).reshape(len(ref["cov"]), 9).max(axis=1) / np.abs(ref["cov"]).reshape(len(ref["cov"]), 9).max(axis=1)
    assert e.max() <= 1e-9, f"{what}: covariances {e.max():.2e}"


@pytest.mark.parametrize("res", RES)
def test_oracle_voxel_stage_equals_the_reference(orc, clouds, res):
    T_lin = _pose(0.02, -0.01, 0.012, [0.08, -0.05, 0.03])
    T_err = _pose(0.021, -0.011, 0.0115, [0.085, -0.047, 0.028])
    sets = dict(clouds)
    sets["walls"] = _walls(res)
    for name, (tgt, src) in sets.items():
        off = FAR.astype(np.float64) if name == "far" else np.zeros(3)
        Tl, Te = T_lin.copy(), T_err.copy()
        # (the far copy: the same motion about its own origin, T' = S T S^-1 with S the translation by FAR)
        Tl[:3, 3] += off - Tl[:3, :3] @ off
        Te[:3, 3] += off - Te[:3, :3] @ off
        for reg in (orc.REG_PLANE, orc.REG_MIN_EIG):
            for mode in vr.MODES:
                tables = {}
                for method in vr.METHODS:
                    what = f"{name} res={res} reg={reg} {mode} {method}"
                    o = _oracle(orc, tgt, src, res, method, mode, reg)
                    tc, sc = o.target_cov(len(tgt)), o.source_cov(len(src))
                    ref = tables.get("ref") or vr.voxel_table(tgt, tc, res, mode)
                    tables["ref"] = ref
                    _check_table(o.voxelmap(), ref, what, 1e-9 if mode == "MULTIPLICATIVE" else 1e-12)
                    cost, H, b = o.linearize(Tl)
                    rcost, rH, rb, corr = vr.linearize(src, sc, ref, Tl, res, method)
                    assert o.num_correspondences == len(corr["src"]), f"{what}: {o.num_correspondences} vs {len(corr['src'])} correspondences"
                    assert vr.rel(cost, rcost) <= 1e-9 and vr.rel(H, rH) <= 1e-9 and vr.rel(b, rb) <= 1e-9, \
                        f"{what}: cost {vr.rel(cost, rcost):.1e} H {vr.rel(H, rH):.1e} b {vr.rel(b, rb):.1e}"
                    e = o.compute_error(Te)
                    assert vr.rel(e, vr.compute_error(src, ref, corr, Te)) <= 1e-9, what
                    if mode == "ADDITIVE_WEIGHTED":      # AdditiveGaussianVoxel for both (fast_vgicp_voxel.hpp:129-141): the same bits
                        a = _oracle(orc, tgt, src, res, method, "ADDITIVE", reg)
                        va, vw = a.voxelmap(), o.voxelmap()
                        assert all(np.array_equal(va[k], vw[k]) for k in va), what
                        ca, Ha, ba = a.linearize(Tl)                # (the oracle's OpenMP reduction order varies from call to call)
                        assert a.num_correspondences == o.num_correspondences, what
                        assert vr.rel(ca, cost) <= 1e-12 and vr.rel(Ha, H) <= 1e-12 and vr.rel(ba, b) <= 1e-12, what
                    if name == "synthetic" and method == "DIRECT1":
                        assert len(corr["src"]) > 0.3 * len(src), (what, len(corr["src"]))
                    if name == "synthetic" and method != "DIRECT1":
                        n1 = len(vr.correspondences(src, sc, ref, Tl, res, "DIRECT1")["src"])
                        assert len(corr["src"]) > n1, what            # the offsets find voxels the own cell does not


def test_wall_points_are_sharp():
    """The constructions decide at the last bit.  At the six resolutions above x / res and x * (1 / res) give the same floor for every
    fp32 value within an ulp of a wall (searched over 400 000 cells of each); where the wall (c + 0.5) * res is itself a binary
    fraction at a non-binary resolution (c = 7, 12, ... at 1.1 and 1.3) they do not, and those are the walls the GPU tests use to tell
    the two apart."""
    assert vr.wall_sharpness(1.1, [7, 12, 22, 27, 47, 52, 57]) >= 0.14
    assert vr.wall_sharpness(1.3, [7, 12, 22, 27, 42, 47, 52, 57]) >= 0.14
    for res in RES:
        x = vr.wall_values(res, WALL_CELLS)
        c = vr.floor_div(x, res)
        # every wall is straddled: its own value and +-1..3 ulps land on both sides
        for j, cell in enumerate(WALL_CELLS):
            cj = c[j::len(WALL_CELLS)]
            assert cj.min() == cell - 1 and cj.max() == cell, (res, cell, cj)
    from scipy.spatial.transform import Rotation
    R = Rotation.from_rotvec([0.3, -0.2, 0.5]).as_matrix()
    rng = np.random.default_rng(11)
    p, T, walls, share = vr.wall_sources(0.3, R, np.arange(-8, 8), rng)
    assert share >= 0.2, share                        # another summation order of the pose product moves a fifth of them
    for j in range(len(p)):
        q = vr.transform(T[j], p[j:j + 1])[0]
        assert np.array_equal(np.floor(q / 0.3 - 0.5).astype(np.int64), walls[j])


def test_reference_against_a_literal_loop(orc):
    """the vectorised reference against a plain per-correspondence loop over the reference's statements, on a small cloud"""
    rng = np.random.default_rng(3)
    tgt = rng.uniform(-2.0, 2.0, (400, 3)).astype(np.float32)
    src = rng.uniform(-2.0, 2.0, (60, 3)).astype(np.float32)
    tc, sc = orc.covariances_m(tgt, orc.REG_MIN_EIG, k=10), orc.covariances_m(src, orc.REG_MIN_EIG, k=10)
    T = _pose(0.1, 0.05, -0.02, [0.1, 0.2, -0.1])
    res = 0.7
    for mode in ("ADDITIVE", "MULTIPLICATIVE"):
        table = vr.voxel_table(tgt, tc, res, mode)
        vox = {}
        for i, p in enumerate(tgt.astype(np.float64)):
            c = tuple(int(np.floor(p[a] / res - 0.5)) for a in range(3))
            v = vox.setdefault(c, dict(n=0, m=np.zeros(4), C=np.zeros((4, 4))))
            v["n"] += 1
            C4 = np.zeros((4, 4)); C4[:3, :3] = tc[i]
            if mode == "ADDITIVE":
                v["m"] += np.append(p, 1.0); v["C"] += C4
            else:
                C4[3, 3] = 1.0
                Ci = np.linalg.inv(C4)
                v["C"] += Ci; v["m"] += Ci @ np.append(p, 1.0)
        for v in vox.values():
            if mode == "ADDITIVE":
                v["m"] /= v["n"]; v["C"] /= v["n"]
            else:
                v["C"][3, 3] = 1.0; v["m"][3] = 1.0
                v["C"] = np.linalg.inv(v["C"]); v["m"] = v["C"] @ v["m"]
        keys = sorted(vox, key=lambda c: (c[2], c[1], c[0]))
        assert np.array_equal(table["coords"], np.array(keys))
        assert np.allclose(table["mean"], [vox[c]["m"][:3] for c in keys], rtol=0, atol=1e-12)
        assert np.allclose(table["cov"], [vox[c]["C"][:3, :3] for c in keys], rtol=1e-12, atol=0)
        for method in vr.METHODS:
            cost, H, b, corr = vr.linearize(src, sc, table, T, res, method)
            lc, lH, lb, n = 0.0, np.zeros((6, 6)), np.zeros(6), 0
            for i, p in enumerate(src.astype(np.float64)):
                q = T[:3, :3] @ p + T[:3, 3]
                c = np.floor(q / res - 0.5).astype(int)
                for o in vr.OFFSETS[method]:
                    v = vox.get(tuple(int(x) for x in c + o))
                    if v is None:
                        continue
                    n += 1
                    C4 = np.zeros((4, 4)); C4[:3, :3] = sc[i]
                    RCR = v["C"] + T @ C4 @ T.T
                    RCR[3, 3] = 1.0
                    M = np.linalg.inv(RCR); M[3, 3] = 0.0
                    e = v["m"] - np.append(q, 1.0)
                    w = np.sqrt(v["n"])
                    J = np.zeros((4, 6))
                    J[:3, :3] = [[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]]
                    J[:3, 3:] = -np.eye(3)
                    lc += w * e @ M @ e; lH += w * J.T @ M @ J; lb += w * J.T @ M @ e
            assert n == len(corr["src"]), (mode, method)
            assert vr.rel(cost, lc) <= 1e-10 and vr.rel(H, lH) <= 1e-10 and vr.rel(b, lb) <= 1e-10, (mode, method)
