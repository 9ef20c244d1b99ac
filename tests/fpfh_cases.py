"""Designed clouds for the FPFH descriptors (rgc_fpfh_estimate): every case is dict(name, cloud (n, 3) float32 -- the queries --, surface (None: the cloud
itself), normals (one float32 row per surface point), radius, cells, minima) -- cells: explicit cell sizes of the call's grid tried beside the automatic rule,
minima: what the REFERENCE ALONE proves the case contains (tests/test_fpfh_reference.py checks them on the CPU, with the cap on undecided pairs).  The GPU
tests (tests/test_gpu_fpfh.py) compare the product with the reference on every point.  The shapes are the smallest at which each thing can still go wrong.

  lattice_16   8 x 8 x 8 dyadic lattice (spacing 2^-6 m) with axis-aligned +- normals, radius 1.6 steps: 7392 ordered pairs, every swap decision an exact tie
  lattice_201  or an exact inequality, every vn == 0 exact, no bin coordinate near an interior wall; and radius 2.01 steps (the second shell)
  sphere       3000 points on a noisy unit sphere with perturbed radial normals, r = 0.2
  plane        3000 points on a noisy plane with perturbed normals, r = 0.12
  plane_nan    the same with 5 % invalid normals (a NaN row, a single NaN or an infinite component): skipped pair by pair, an invalid point's SPFH is zero
  dups         400 points with 40 exact duplicates (key 0: skipped, but counted in m) and 20 isolated points (m = 1: SPFH zero, their FPFH rows zero)
  keypoints    64 queries that are not surface points against a 4000-point surface: the mark / compact route, n_spfh < n_surface, one query with an empty row
  blob         3000 points all within one radius: counts in the thousands, rows of 3000 members
  big          20 000 points on a wavy sheet: LDS rows reused across many workgroups
  one_cell     300 points in a 0.2 m box on a grid of 64 m cells: everything in one cell"""
import functools

import numpy as np

STEP = 2.0 ** -6


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _case(name, cloud, normals, radius, surface=None, cells=(), **minima):
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(name=name, cloud=f32(cloud), surface=None if surface is None else f32(surface), normals=f32(normals), radius=float(radius), cells=tuple(cells), minima=minima)


def _lattice():
    rng = np.random.default_rng(2601)
    I = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3)
    I = I[rng.permutation(len(I))]
    N = np.zeros((len(I), 3))
    N[np.arange(len(I)), I.sum(axis=1) % 3] = np.where((3 * I[:, 0] + 5 * I[:, 1] + 7 * I[:, 2]) % 4 < 2, 1.0, -1.0)
    return I * STEP + np.array([1.0, -0.5, 0.25]), N


def _sphere():
    rng = np.random.default_rng(2602)
    v = _unit(rng.normal(0, 1, (3000, 3)))
    return v * (1 + 0.005 * rng.normal(0, 1, (3000, 1))), _unit(v + 0.05 * rng.normal(0, 1, (3000, 3)))


def _plane(seed=2603, n=3000, ext=1.0):
    rng = np.random.default_rng(seed)
    P = np.concatenate([rng.uniform(-ext, ext, (n, 2)), 0.005 * rng.normal(0, 1, (n, 1))], axis=1)
    return P, _unit(np.array([0.0, 0.0, 1.0]) + 0.05 * rng.normal(0, 1, (n, 3)))


def _plane_nan():
    P, N = _plane()
    rng = np.random.default_rng(2604)
    bad = rng.choice(len(P), len(P) // 20, replace=False)
    N[bad[:50]] = np.nan
    N[bad[50:100], rng.integers(0, 3, 50)] = np.nan
    N[bad[100:], rng.integers(0, 3, len(bad) - 100)] = np.inf
    return P, N


def _dups():
    rng = np.random.default_rng(2605)
    P = rng.uniform(-0.3, 0.3, (340, 3))
    P = np.concatenate([P, P[:40], np.stack([5.0 + 3.0 * np.arange(20), np.full(20, -7.0), np.linspace(0, 4, 20)], axis=1)])
    N = _unit(rng.normal(0, 1, (len(P), 3)))
    o = rng.permutation(len(P))
    return P[o], N[o]


def _keypoints():
    S, N = _plane(2606, 4000)
    rng = np.random.default_rng(2607)
    Q = np.concatenate([rng.uniform(-0.5, 0.5, (63, 2)), 0.01 * rng.normal(0, 1, (63, 1))], axis=1)
    Q = np.concatenate([Q[:20], [[30.0, 30.0, 5.0]], Q[20:]])      # one query far from everything: an empty row
    return Q, S, N


def _blob():
    rng = np.random.default_rng(2608)
    v = _unit(rng.normal(0, 1, (3000, 3))) * (0.05 * rng.uniform(0, 1, (3000, 1)) ** (1 / 3))
    return v + np.array([2.0, 1.0, -1.0]), _unit(rng.normal(0, 1, (3000, 3)))


def _big():
    rng = np.random.default_rng(2609)
    xy = rng.uniform(-2.6, 2.6, (20000, 2))
    z = 0.2 * np.sin(2 * xy[:, 0]) * np.cos(2 * xy[:, 1])
    N = np.stack([-0.4 * np.cos(2 * xy[:, 0]) * np.cos(2 * xy[:, 1]), 0.4 * np.sin(2 * xy[:, 0]) * np.sin(2 * xy[:, 1]), np.ones(20000)], axis=1)
    return np.concatenate([xy, z[:, None]], axis=1), _unit(N + 0.03 * rng.normal(0, 1, (20000, 3)))


def _one_cell():
    rng = np.random.default_rng(2610)
    return rng.uniform(-0.1, 0.1, (300, 3)) + np.array([3.0, -1.0, 0.5]), _unit(rng.normal(0, 1, (300, 3)))


@functools.lru_cache(maxsize=None)
def all_cases():
    lat, lat_n = _lattice()
    kq, ks, kn = _keypoints()
    return [
        _case("lattice_16", lat, lat_n, 1.6 * STEP, cells=(STEP, 0.25), pairs=7392, vn0=1792, ties=4032, undecided_max=0),
        _case("lattice_201", lat, lat_n, 2.01 * STEP, cells=(4 * STEP,), pairs=12440, vn0=3328, ties=7544, undecided_max=0),
        _case("sphere", *_sphere(), 0.2, cells=(0.0625, 0.25, 1.0), pairs=85000, swaps=35000),
        _case("plane", *_plane(), 0.12, cells=(0.0625, 0.25, 1.0), pairs=90000, swaps=35000),
        _case("plane_nan", *_plane_nan(), 0.12, pairs=80000, invalid_members=4000),
        _case("dups", *_dups(), 0.12, cells=(0.03125,), key0=80, isolated=20),
        _case("keypoints", kq, kn, 0.12, surface=ks, cells=(0.0625, 0.5), empty_rows=1, n_spfh_max=2000, n_spfh_min=500),
        _case("blob", *_blob(), 0.12, cells=(0.03125,), pairs=8_990_000, max_count=1500, max_members=3000),
        _case("big", *_big(), 0.12, pairs=600000),
        _case("one_cell", *_one_cell(), 0.05, cells=(64.0,), pairs=3000),
    ]


def cases():
    return {c["name"]: c for c in all_cases()}


def surface_of(case):
    return case["cloud"] if case["surface"] is None else case["surface"]


@functools.lru_cache(maxsize=None)
def ref(name):
    """the reference of a case, computed once and shared by the tests that need it (never modified)"""
    import fpfh_reference as fr
    c = cases()[name]
    return fr.estimate(c["cloud"], c["normals"], c["radius"], c["surface"])
