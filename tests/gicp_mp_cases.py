"""Designed inputs for FastGICPMultiPoints (rgc_gicpmp_*): every case is dict(name, tgt, src, r, poses, minima) -- `minima` are lower bounds of
gicp_mp_reference.census over all the case's poses, met by the REFERENCE ALONE (tests/test_gicp_mp_reference.py checks that on the CPU); the GPU tests
(tests/test_gpu_gicp_mp.py) compare the product with the reference on every query of every case.

  scene_r*   the 24 k map / 8 k scan of tests/test_gpu_gicp.py's `data` fixture (the same generator calls) plus 200 source points moved outside the map so
             that empty rows exist, at radii 0.01, 0.25, 0.5, 1.0 and 2.5 (the last reaches three cells of the 1 m grid either way)
  dyadic_r*  coordinates on the 2^-6 m lattice about (100, -60, 2), lattice translations and 90 degree turns as poses: every key is exact in fp32.  Around
             chosen queries targets sit ON the gate (key == r2: excluded by the strict rule), on the last lattice shell inside it, on the one before, and on
             the query itself (w = 1), with their permutations and signs.  r = 0.5 (gate 1024 / 4096: shells 1022 -- raw weight 0.00098, the 1e-3 clamp
             active -- and 1021; 1023 is no sum of three squares), 0.375 (576: 574, 573) and 0.625 (1600: 1598, 1597)
  ulp_shell  one query, targets whose fp32 keys are r2 itself and the floats next to it on either side (found by search with the reference's key)
  outside    queries outside the target's box by less than r (neighbours exist) and by more than r (none)
  one_cell   a target inside one grid cell
  whole_*    a radius larger than the map: every row is the whole target, at 65 and 577 target points
  tiny_*     targets of 2, 3 and 65 points"""
import functools
import itertools

import numpy as np

import gicp_mp_reference as mr
import ndt_reference as nr
import nn_reference as nn

CENTER = (100.0, -60.0, 2.0)
SCENE_RADII = (0.01, 0.25, 0.5, 1.0, 2.5)
DYADIC_RADII = (0.5, 0.375, 0.625)


@functools.lru_cache(maxsize=None)
def scene_data():
    """tests/test_gpu_gicp.py's `data` fixture, call for call, then 200 source points moved 40 m away from the map"""
    rng = np.random.default_rng(9101)
    tgt = nr.scene(rng, 24000)
    T = nr.random_pose(rng, about=CENTER)
    Ti = np.linalg.inv(T)
    src = (nr.scene(rng, 8000).astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(0, 0.01, (8000, 3))).astype(np.float32)
    poses = [np.eye(4), T] + [nr.random_pose(rng, about=CENTER) for _ in range(3)]
    far = src[:200].copy()
    far[:, 0] += np.float32(40.0)
    far[:, 2] += np.float32(15.0)
    return dict(tgt=tgt, src=np.concatenate([src, far]), T=T, poses=poses)


def scene_case(r):
    d = scene_data()
    minima = {0.01: dict(q0=7000, q1=1), 0.25: dict(q0=200, q1=50, q2_63=5000), 0.5: dict(q0=200, q2_63=6000), 1.0: dict(q0=200, q2_63=1000, q64=1000),
              2.5: dict(q0=200, q64=7500, clamped=100, on_r2=0)}[r]
    return dict(name="scene_r%g" % r, tgt=d["tgt"], src=d["src"], r=r, poses=[d["T"], np.eye(4)] if r < 2.5 else [d["T"]], minima=minima)


def _shell(n2, lim):
    """every integer triple with x^2 + y^2 + z^2 == n2 (permutations and signs included)"""
    out = []
    for x, y, z in itertools.product(range(-lim, lim + 1), repeat=3):
        if x * x + y * y + z * z == n2:
            out.append((x, y, z))
    return out


def dyadic_shells(r):
    """(gate, last shell inside, the one before) in squared lattice units, the latter two found as the largest sums of three squares below the gate"""
    R = int(round(r / nn.STEP))
    assert R * nn.STEP == r
    gate = R * R
    inside = []
    n2 = gate - 1
    while len(inside) < 2:
        if _shell(n2, R):
            inside.append(n2)
        n2 -= 1
    return gate, inside[0], inside[1]


def dyadic_case(r):
    gate, s1, s2 = dyadic_shells(r)
    R = int(round(r / nn.STEP))
    rng = np.random.default_rng(int(r * 1000))
    c = np.round(np.array(CENTER) / nn.STEP).astype(np.int64)
    # poses under which lattice points stay lattice points: the identity, a lattice translation, a quarter turn about z through the centre plus a step
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.int64)
    lat_poses = [(np.eye(3, dtype=np.int64), np.zeros(3, np.int64)), (np.eye(3, dtype=np.int64), np.array([3, -2, 1])), (Rz, c - Rz @ c + np.array([1, 0, -1]))]
    poses = []
    for Ri, ti in lat_poses:
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Ri, ti * nn.STEP
        poses.append(T)
    # designed queries 4 m apart (no two share a neighbour); the source holds, for every pose, the points that pose moves ONTO them, plus a lattice
    # filler of random targets and queries
    Q = c + np.array([[0, 0, 0], [256, 0, 0], [0, 256, 64], [-256, -256, 0]])
    offs = np.array(_shell(gate, R) + _shell(s1, R) + _shell(s2, R) + [(0, 0, 0)], np.int64)
    It = np.concatenate([q + offs for q in Q[:3]] + [c + rng.integers(-400, 400, (3000, 3))])
    It = np.unique(It, axis=0)
    Iq = np.concatenate([(Q - ti) @ Ri for Ri, ti in lat_poses] + [c + rng.integers(-400, 400, (1500, 3))])      # (Q - t) R = R^T (Q - t) row by row
    tgt, src = nn.lattice(It), nn.lattice(Iq)
    n_on, n1, n2 = len(_shell(gate, R)), len(_shell(s1, R)), len(_shell(s2, R))
    # per pose three designed queries: the gate shell, the two shells inside it and the coincident target each
    return dict(name="dyadic_r%g" % r, tgt=tgt, src=src, r=r, poses=poses, gate=gate, shells=(s1, s2),
                minima=dict(on_r2=9 * n_on, w_one=9, clamped=(9 * n1 if r == 0.5 else 0), q0=3),
                key_counts={gate: 9 * n_on, s1: 9 * n1, s2: 9 * n2, 0: 9})


@functools.lru_cache(maxsize=None)
def ulp_shell_case():
    r = 0.5
    r2 = mr.r2_of(r)
    rng = np.random.default_rng(4242)
    q = np.float32([[100.0, -60.0, 2.0]])
    u = rng.normal(size=(400000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    cand = (q.astype(np.float64) + r * u).astype(np.float32)
    key = mr.fp32_keys(np.repeat(q, len(cand), 0), cand)
    want = [np.nextafter(r2, np.float32(0)), r2, np.nextafter(r2, np.float32(np.inf))]
    picks = [np.flatnonzero(key == k)[:8] for k in want]
    tgt = np.concatenate([cand[p] for p in picks] + [cand[:40]])
    src = np.concatenate([q, q + np.float32([[0.25, 0, 0]])])
    return dict(name="ulp_shell", tgt=tgt, src=src, r=r, poses=[np.eye(4)], minima=dict(on_r2=4, step_inside=4, step_outside=4))


def _box_target(rng, n, half=2.0):
    return (np.array(CENTER) + rng.uniform(-half, half, (n, 3))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def geometry_cases():
    rng = np.random.default_rng(606)
    out = []
    tgt = _box_target(rng, 4000)
    face = np.array(CENTER) + np.stack([np.full(300, 2.0), rng.uniform(-2, 2, 300), rng.uniform(-2, 2, 300)], 1)
    near, far = face + [0.3, 0, 0], face + [0.8, 0, 0]
    corner = np.array(CENTER) + rng.choice([-1.0, 1.0], (100, 3)) * (2.0 + rng.uniform(0.05, 0.2, (100, 3)))
    out.append(dict(name="outside", tgt=tgt, src=np.concatenate([near, far, corner]).astype(np.float32), r=0.5, poses=[np.eye(4)],
                    minima=dict(q0=300, q2_63=100)))
    cell = (np.array([100.7, -59.8, 2.2]) + rng.uniform(-0.15, 0.15, (500, 3))).astype(np.float32)      # inside the 1 m cell [100.5, 101.5) x [-60.5, -59.5) x [1.5, 2.5)
    srcc = (np.array([100.7, -59.8, 2.2]) + rng.uniform(-0.6, 0.6, (700, 3))).astype(np.float32)
    out.append(dict(name="one_cell", tgt=cell, src=srcc, r=0.25, poses=[np.eye(4)], minima=dict(q0=50, q64=50, q2_63=50)))
    for n in (65, 577):
        t = _box_target(rng, n, 1.5)
        s = _box_target(rng, 300, 1.5)
        out.append(dict(name="whole_%d" % n, tgt=t, src=s, r=8.0, poses=[np.eye(4), nr.random_pose(rng, about=CENTER)], minima=dict(q64=300), whole=True))
    for n in (2, 3, 65):
        t = _box_target(rng, n, 0.5)
        s = _box_target(rng, 400, 0.8)
        out.append(dict(name="tiny_%d" % n, tgt=t, src=s, r=0.5, poses=[np.eye(4)], minima=dict(q0=1, q1=1) if n < 65 else dict(q2_63=50), k=2))
    return out


def all_cases():
    return [scene_case(r) for r in SCENE_RADII] + [dyadic_case(r) for r in DYADIC_RADII] + [ulp_shell_case()] + list(geometry_cases())


@functools.lru_cache(maxsize=None)
def rows_of(name, pose_index):
    """the reference's rows of a case at one of its poses, computed once and shared (read-only)"""
    case = {c["name"]: c for c in all_cases()}[name]
    q = nn.transform_f32(case["src"], np.asarray(case["poses"][pose_index], np.float64).astype(np.float32))
    rw = mr.radius_rows(case["tgt"], q, case["r"])
    for v in rw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return rw


def census_of(case):
    """the census summed over the case's poses"""
    tot = {}
    for p in range(len(case["poses"])):
        for k, v in mr.census(rows_of(case["name"], p), case["r"]).items():
            tot[k] = max(tot.get(k, 0), v) if k == "max_row" else tot.get(k, 0) + v
    return tot
