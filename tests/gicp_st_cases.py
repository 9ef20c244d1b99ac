"""Designed inputs for FastGICPSingleThread (rgc_gicpst_*): every case is dict(name, tgt, src, cov_t, cov_s, d_max, steps, minima).  `steps` is a list
of 4x4 poses and the string "reset"; `minima` are lower bounds of `census` over the case's steps, met by the REFERENCE ALONE
(tests/test_gicp_st_reference.py checks that on the CPU); the GPU tests (tests/test_gpu_gicp_st.py) compare the product with the reference after every
step of every case.  The covariances are user-set and of the PLANE form I - 0.999 n n^T (eigenvalues 1e-3, 1, 1) with designed unit normals: lattices
and tiny clouds make kNN covariances degenerate.  The target's search grid has 1 m cells with walls at integer + 0.5 (the context's default resolution).

  sizes_N      source sizes at the wave and workgroup edges of the compaction (63, 64, 65, 255, 256, 257, 513; one point is not a cloud the context
               accepts) against a 4000-point box; steps T0, T0 again (d = 0: every untied point is skipped), a step of 8 cm (mixed), a step of 3.3 m
               (several cells: everything is searched)
  two_points   a target of two points (key2 = the distance to the other one)
  duplicates   every target point twice: key1 == key2 everywhere, every point searched at every step
  lattice_ties a 0.5 m dyadic lattice target and queries at its cell centres: eight exact nearest ties each, always searched; corr = the smallest index
  walls        queries 0.1 m inside their cell whose nearest is in the own cell and whose second nearest lies across a wall, an edge and a corner -- with a
               second own-cell point FARTHER than the outside one (the own-cell exit and the ball pruning must bound the second), and with the nearest
               alone in its cell
  outside      queries up to 6 m outside the target's box
  sparse       40 target points in a 40 x 40 x 10 m box, queries all over it: the cube grows more than twice before it holds two points
  sticky       target points at x = 0 and x = 10, d_max = 1, source points at x = 0.9 and x = -1.1 moved by +0.2 m: both are skipped, the first stays kept
               at 1.1 m, the second stays at -1 at 0.9 m; after a reset both flip
  stale_M      eight source points offset 0.1 m per axis from the origin of a 1 m target lattice, a 5 degree turn about z between two linearisations:
               all skipped (0.173 + 0.044 < 0.911 - 0.044), every M is the one of the first pose"""
import functools

import numpy as np

import gicp_st_reference as sr
import nn_reference as nn

SIZES = (63, 64, 65, 255, 256, 257, 513)
BASE = np.array([20.0, -12.0, 3.0])


def plane_cov(normals):
    n = np.asarray(normals, np.float64)
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    return np.eye(3) - 0.999 * np.einsum("ni,nj->nij", n, n)


def _normals(rng, n, about=None, spread=0.3):
    """unit normals: random, or within `spread` of the direction `about`"""
    v = rng.normal(size=(n, 3)) if about is None else np.asarray(about, np.float64) + spread * rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def translation(x, y=0.0, z=0.0):
    T = np.eye(4)
    T[:3, 3] = [x, y, z]
    return T


def rot_z(deg, about=(0.0, 0.0, 0.0)):
    a, T, c = np.deg2rad(deg), np.eye(4), np.asarray(about, np.float64)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = c - T[:3, :3] @ c
    return T


def _case(name, tgt, src, steps, rng, d_max=sr.FLT_MAX, minima=None, normals_t=None, normals_s=None):
    tgt, src = np.asarray(tgt, np.float32), np.asarray(src, np.float32)
    return dict(name=name, tgt=tgt, src=src, cov_t=plane_cov(_normals(rng, len(tgt)) if normals_t is None else normals_t),
                cov_s=plane_cov(_normals(rng, len(src)) if normals_s is None else normals_s), d_max=float(d_max), steps=steps, minima=minima or {})


@functools.lru_cache(maxsize=None)
def box_target():
    rng = np.random.default_rng(7301)
    return (BASE + rng.uniform([-5, -5, -2], [5, 5, 2], (4000, 3))).astype(np.float32)


def sizes_case(n):
    rng = np.random.default_rng(7400 + n)
    tgt = box_target()
    src = tgt[rng.choice(len(tgt), n, replace=False)].astype(np.float64) + rng.normal(0, 0.02, (n, 3))
    T0 = rot_z(0.4, BASE) @ translation(0.01, -0.02, 0.005)
    steps = [T0, T0, translation(0.08, 0.0, 0.0) @ T0, translation(3.3, -2.2, 1.1) @ T0]
    # per step: (searched, skipped) bounds are asserted exactly by the tests (n, 0 / 0, n / mixed / n, 0); the totals below follow from them
    return _case("sizes_%d" % n, tgt, src, steps, rng, d_max=0.5, minima=dict(searched=2 * n + 1, skipped=n + 1))


def two_points_case():
    rng = np.random.default_rng(7501)
    tgt = BASE + np.array([[0.0, 0.0, 0.0], [1.75, 0.5, -0.25]])
    src = BASE + rng.uniform(-2, 3, (100, 3))
    T0 = np.eye(4)
    return _case("two_points", tgt, src, [T0, T0, translation(0.05, 0.02, 0.0), translation(4.0, 4.0, 1.0)], rng, minima=dict(searched=101, skipped=101))


def duplicates_case():
    rng = np.random.default_rng(7502)
    half = box_target()[:300]
    tgt = np.concatenate([half, half])
    src = half[:130].astype(np.float64) + rng.normal(0, 0.03, (130, 3))
    T0 = translation(0.01, 0.0, 0.0)
    return _case("duplicates", tgt, src, [T0, T0, translation(0.02, 0.0, 0.0)], rng, minima=dict(searched=390, skipped=0, tied=390))


def lattice_ties_case():
    rng = np.random.default_rng(7503)
    g = np.arange(-3, 4)
    I = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    tgt = nn.lattice(I * 32 + np.array([1280, -768, 192]))                       # 0.5 m pitch about (20, -12, 3)
    cells = I[(np.abs(I) < 3).all(axis=1)][::3]
    src = nn.lattice(cells * 32 + 16 + np.array([1280, -768, 192]))              # cell centres: eight corners at the same exact key
    T0 = np.eye(4)
    return _case("lattice_ties", rng.permutation(tgt), src, [T0, T0, translation(0.5, 0.0, 0.0)], rng, minima=dict(searched=3 * len(src), skipped=0, tied=3 * len(src)))


def walls_case():
    rng = np.random.default_rng(7504)
    tgt, src = [], []
    dirs = {"wall": (1, 0, 0), "edge": (1, 1, 0), "corner": (1, 1, 1)}
    for b, (kind, u) in enumerate(dirs.items()):
        for variant in range(2):
            for sign in (1, -1):
                u_ = sign * np.array(u, np.float64)
                cell = np.array([10.0 + 4 * b, 2.0 + 4 * variant, 1.0 + 3 * (sign < 0)])       # the cell [cell - 0.5, cell + 0.5)^3
                q = cell + u_ * 0.4                                                             # 0.1 m inside the wall(s) along u
                inward = -u_ / np.linalg.norm(u_)
                tgt.append(q + 0.05 * inward)                                                   # the nearest: own cell
                tgt.append(q + u_ * 0.11)                                                       # the second nearest: across the wall / edge / corner
                if variant == 0:
                    tgt.append(q + 0.4 * inward)                                                # a second own-cell point, farther than the outside one
                src.append(q)
    tgt += list(np.array([0.0, 0.0, 0.0]) + rng.uniform([0, 0, 0], [24, 8, 6], (60, 3)))        # a thin background: the grid spans the whole block
    return _case("walls", np.array(tgt), np.array(src), [np.eye(4), translation(0.001, 0.0, 0.0)], rng, minima=dict(searched=12, skipped=12))


def outside_case():
    rng = np.random.default_rng(7505)
    tgt = box_target()[:1500]
    lo, hi = tgt.min(0).astype(np.float64), tgt.max(0).astype(np.float64)
    src = []
    for s in np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(-1, 3):
        if s.any():
            for far in (0.3, 2.5, 6.0):
                c = np.where(s < 0, lo - far, np.where(s > 0, hi + far, rng.uniform(lo, hi)))
                src.append(c)
    return _case("outside", tgt, np.array(src), [np.eye(4), translation(0.0, 0.01, 0.0), translation(0.5, 0.5, 0.5)], rng, minima=dict(searched=78 + 1, skipped=1))


def sparse_case():
    rng = np.random.default_rng(7506)
    tgt = BASE + rng.uniform([-20, -20, -5], [20, 20, 5], (40, 3))
    src = BASE + rng.uniform([-24, -24, -7], [24, 24, 7], (200, 3))
    return _case("sparse", tgt, src, [np.eye(4), np.eye(4), translation(1.5, -1.0, 0.5)], rng, minima=dict(searched=201, skipped=201))


def sticky_case():
    rng = np.random.default_rng(7507)
    tgt = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0]])
    src = np.array([[0.9, 0.0, 0.0], [-1.1, 0.0, 0.0]])
    move = translation(0.2)
    return _case("sticky", tgt, src, [np.eye(4), move, "reset", move], rng, d_max=1.0, minima=dict(searched=4, skipped=2, kept_beyond=1, minus_within=1))


def stale_case():
    rng = np.random.default_rng(7508)
    g = np.arange(-3, 4)
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    src = 0.1 * np.stack(np.meshgrid([-1, 1], [-1, 1], [-1, 1], indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    # normals near the x axis on both clouds: S = C_B + R C_A R^T is thin along x at the first pose, and a turn about z opens it
    nt, ns = _normals(rng, len(tgt), about=(1, 0, 0), spread=0.05), _normals(rng, len(src), about=(1, 0, 0), spread=0.05)
    return _case("stale_M", tgt, src, [translation(0.02, 0.01, 0.0), rot_z(5.0) @ translation(0.02, 0.01, 0.0)], rng, normals_t=nt, normals_s=ns,
                 minima=dict(searched=8, skipped=8, stale=8))


def designed_cases():
    return [sizes_case(n) for n in SIZES] + [two_points_case(), duplicates_case(), lattice_ties_case(), walls_case(), outside_case(), sparse_case(),
                                             sticky_case(), stale_case()]


def make_reference(case):
    ref = sr.GICPST(case["d_max"])
    ref.set_target(case["tgt"], case["cov_t"])
    ref.set_source(case["src"], case["cov_s"])
    return ref


def census(ref, T, first, R_searched):
    """what one linearisation at T left behind, from the reference's state alone.  R_searched: per point the rotation it was last searched under
    (updated here).  searched / skipped count only linearisations that had anchors (`first` is False)."""
    st = ref.state
    q = nn.transform_f32(ref.source, np.asarray(T, np.float64).astype(np.float32))
    _, now1, _ = sr.two_nearest(ref.target, q)
    d2 = ref.d_max * ref.d_max
    kept = st["corr"] >= 0
    to_pair = np.where(kept, sr.keys_f32(q, ref.target)[np.arange(len(q)), np.maximum(st["corr"], 0)], np.float32(0)).astype(np.float64)
    R = np.asarray(T, np.float64)[:3, :3]
    R_searched[st["searched"]] = R
    stale = kept & ~st["searched"] & (np.abs(R_searched - R).max(axis=(1, 2)) > 1e-6)
    return dict(searched=int(st["searched"].sum()), skipped=0 if first else int((~st["searched"]).sum()),
                kept_beyond=int((kept & (to_pair >= d2)).sum()), minus_within=int((~kept & (now1.astype(np.float64) < d2)).sum()),
                stale=int(stale.sum()), tied=int((st["key1"] == st["key2"]).sum()))


def run_reference(case, each=None):
    """the case's steps on a fresh reference; each(ref, T, sums) after every linearisation.  Returns (ref, totals of census)"""
    ref = make_reference(case)
    R_searched = np.zeros((len(case["src"]), 3, 3))
    total, first = {}, True
    for step in case["steps"]:
        if isinstance(step, str):
            ref.reset()
            first = True
            continue
        sums = ref.linearize(step)
        for k, v in census(ref, step, first, R_searched).items():
            total[k] = total.get(k, 0) + v
        first = False
        if each:
            each(ref, step, sums)
    return ref, total
