"""Designed clouds for surface normal estimation (rgc_normal_estimate): every case is dict(name, cloud (n, 3) float32 -- the queries --, surface (None: the cloud
itself), runs, cells, minima) -- runs: settings dict(k | radius, vp, flip) of the call, cells: explicit cell sizes of the call's grid tried beside the
automatic rule, minima: what the REFERENCE ALONE proves the case contains (tests/test_normal_reference.py checks them on the CPU).  The GPU tests
(tests/test_gpu_normals.py) compare the product with the reference on every query.

  sheet        4 000 points uniform in [-1, 1]^2, z = 0.01 N(0, 1), k = 12 and r = 0.15: every query decided, no relative gap under 1e-2; the viewpoint at the
               origin, inside the cloud, and flip = 0
  sheet_far    the same sheet translated by (1000, -2000, 500): the shifted origin holds the same bound where PCL's unshifted fp32 sums fail
  sweep        a 16-beam sweep (synth.make_world(30), make_scan(n_az=400)), 6 154 points, k = 10 / 20 and r = 0.5 / 1.0: rows under three members (the NaN
               route) and nearly collinear ring neighbourhoods (undecided, at most 5 % of the valid queries)
  lattice      6 x 6 x 6 dyadic lattice (spacing 2^-3): six neighbours tie exactly at ranks 1..6, twelve behind them -- k = 5 and 10 cut inside a tie, the
               row is still unique by index; r = the spacing exactly (neighbours ON the radius are excluded: the point alone, NaN) and r = 0.13
  dups         k + 5 copies of one point: rank 0, the covariance is exactly zero
  pole         an exactly collinear pole on dyadic coordinates: rank 1
  one_cell     300 points in a box of 0.2 m on a grid of 64 m cells: everything in one cell
  walls        points exactly on the walls of 0.5 m cells (coordinates (i + 0.5) / 2), some jittered
  sparse       a 2 000-point sheet and 20 strays 50 to 500 m away whose cubes must grow (info.grown > 0)
  n_1 n_2 n_3  one, two, three points: m < 3 is NaN on both routes; n_3 is the smallest valid row
  short_5 full_8   n_surface < k and n_surface = k at k = 8
  tiers        200 points at k = 3, 4, 5, 8, 9, 16, 17, 32: both sides of every list tier
  n_63 n_64 n_65   workgroup seams (64 queries of four lanes fill a workgroup)
  ball         400 points within 0.2 m, r = 0.5: every ball holds all 400 (more than 256 members)
  alone        the sheet at r = 1e-5: every ball holds the point itself only, every row is NaN
  surface      the sheet as search surface; the queries are its 0.1 m leaf centroids, 30 points outside its bounding box and 20 more than the radius away from
               everything
  plane        a dyadic sheet exactly in z = 0.25 with the viewpoint exactly in that plane (the dot product is exactly 0: the solver's sign stays), below
               it, and flip = 0"""
import functools

import numpy as np

FAR = np.array([1000.0, -2000.0, 500.0])
TIER_K = (3, 4, 5, 8, 9, 16, 17, 32)


def run(k=0, radius=0.0, vp=(0.0, 0.0, 0.0), flip=True):
    return dict(k=k, radius=radius, vp=tuple(float(v) for v in vp), flip=bool(flip))


def _sheet(seed=2502, n=4000):    # (a seed at which the reference finds no relative gap under 1e-2 on either route, near the origin and far from it)
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-1, 1, (n, 2)), 0.01 * rng.normal(0, 1, (n, 1))], axis=1)


def _case(name, cloud, runs, surface=None, cells=(), **minima):
    return dict(name=name, cloud=np.ascontiguousarray(cloud, np.float32), surface=None if surface is None else np.ascontiguousarray(surface, np.float32), runs=tuple(runs),
                cells=tuple(cells), minima=minima)


@functools.lru_cache(maxsize=None)
def sweep_cloud():
    from rgc_slam_amd import synth
    world = synth.make_world(30)
    return np.ascontiguousarray(synth.make_scan(world, np.eye(4), n_az=400)["xyz"], np.float32)


def _lattice():
    rng = np.random.default_rng(2502)
    I = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), axis=-1).reshape(-1, 3)
    return I[rng.permutation(len(I))] * 0.125 + np.array([4.0, -2.0, 1.0])


def _walls():
    rng = np.random.default_rng(2503)
    I = rng.integers(-4, 4, (500, 3))
    P = (I + 0.5) * 0.5                                     # exactly on the walls of cells of 0.5 (the grid's rule: floor(x / cell - 0.5))
    P[250:] += rng.uniform(-0.2, 0.2, (250, 3))
    return np.unique(P, axis=0)[rng.permutation(len(np.unique(P, axis=0)))]


def _sparse():
    rng = np.random.default_rng(2504)
    sheet = np.concatenate([rng.uniform(-5, 5, (2000, 2)), rng.normal(0, 0.01, (2000, 1))], axis=1)
    ang = np.arange(20) * (2 * np.pi / 20)
    rad = np.linspace(50.0, 500.0, 20)
    strays = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.linspace(-20, 20, 20)], axis=1)
    return np.concatenate([sheet, strays])[rng.permutation(2020)]


def _box(seed, n, ext, at=(3.0, -1.0, 0.5)):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (n, 3)) * np.asarray(ext) + np.asarray(at)


def _ball():
    rng = np.random.default_rng(2505)
    v = rng.normal(0, 1, (400, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * (0.1 * rng.uniform(0, 1, (400, 1)) ** (1 / 3)) + np.array([7.0, 7.0, -3.0])


def _surface_queries(sheet):
    rng = np.random.default_rng(2506)
    s32 = sheet.astype(np.float32).astype(np.float64)
    ijk = np.floor(s32 / 0.1).astype(np.int64)
    _, inv = np.unique(ijk, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv)
    cen = np.stack([np.bincount(inv, s32[:, a]) / cnt for a in range(3)], axis=1)
    outside = np.stack([rng.uniform(1.02, 1.12, 30), rng.uniform(-1, 1, 30), rng.normal(0, 0.01, 30)], axis=1)     # beyond x = 1, within reach of the rim
    away = rng.uniform(-1, 1, (20, 3)) * 5 + np.array([40.0, -40.0, 10.0])
    return np.concatenate([cen, outside, away])


def _plane():
    rng = np.random.default_rng(2507)
    xy = rng.integers(-64, 64, (1500, 2)) / 64.0
    xy = np.unique(xy, axis=0)
    return np.concatenate([xy[rng.permutation(len(xy))], np.full((len(xy), 1), 0.25)], axis=1)


@functools.lru_cache(maxsize=None)
def all_cases():
    sheet = _sheet()
    pole = np.stack([np.full(40, 2.5), np.full(40, -1.25), np.arange(40) / 8.0], axis=1)
    tiers = _box(2520, 200, (1, 1, 0.3))
    cs = [
        _case("sheet", sheet, [run(k=12), run(radius=0.15), run(k=12, vp=(0.2, -0.3, 0.0)), run(k=12, flip=False), run(radius=0.15, vp=(0.2, -0.3, 5.0), flip=False)],
              cells=(0.0625, 0.25, 1.0), all_decided=True, min_gap=1e-2),
        _case("sheet_far", sheet + FAR, [run(k=12), run(radius=0.15)], cells=(0.25,), all_decided=True, min_gap=1e-2),
        _case("sweep", sweep_cloud(), [run(k=10), run(k=20), run(radius=0.5), run(radius=1.0)], n=6154, nan_rows={0.5: 2471, 1.0: 116}, max_undecided=0.05),
        _case("lattice", _lattice(), [run(k=5), run(k=10), run(radius=0.125), run(radius=0.13)], cells=(0.25, 4.0), tied_rows=64),
        _case("dups", np.repeat(np.array([[1.5, -2.25, 0.75]]), 13, axis=0), [run(k=8), run(radius=0.5)], cells=(0.25,), rank=0),
        _case("pole", pole, [run(k=6), run(radius=0.4)], cells=(0.25,), rank=1),
        _case("one_cell", _box(2508, 300, (0.1, 0.1, 0.1)), [run(k=10), run(radius=0.05)], cells=(64.0,)),
        _case("walls", _walls(), [run(k=6), run(radius=0.6)], cells=(0.5,)),
        _case("sparse", _sparse(), [run(k=10)], cells=(4.0,), grown=20),
        _case("n_1", _box(2511, 1, (1, 1, 1)), [run(k=3), run(radius=0.5)]),
        _case("n_2", _box(2512, 2, (0.1, 0.1, 0.1)), [run(k=3), run(radius=0.5)]),
        _case("n_3", _box(2513, 3, (0.1, 0.1, 0.1)), [run(k=3), run(radius=0.5)]),
        _case("short_5", _box(2514, 5, (0.3, 0.3, 0.3)), [run(k=8)]),
        _case("full_8", _box(2515, 8, (0.3, 0.3, 0.3)), [run(k=8)]),
        _case("tiers", tiers, [run(k=k) for k in TIER_K], cells=(0.25,)),
        _case("n_63", _box(2563, 63, (1, 1, 0.2)), [run(k=6), run(radius=0.4)]),
        _case("n_64", _box(2564, 64, (1, 1, 0.2)), [run(k=6), run(radius=0.4)]),
        _case("n_65", _box(2565, 65, (1, 1, 0.2)), [run(k=6), run(radius=0.4)]),
        _case("ball", _ball(), [run(radius=0.5)], cells=(0.125,), min_members=257),
        _case("alone", sheet, [run(radius=1e-5)], all_nan=True),
        _case("surface", _surface_queries(sheet), [run(k=10), run(radius=0.15)], surface=sheet, cells=(0.25,), outside=30, empty_rows=20),
        _case("plane", _plane(), [run(k=9, vp=(0.5, 0.25, 0.25)), run(k=9, vp=(0.0, 0.0, -3.0)), run(radius=0.1, vp=(0.5, 0.25, 0.25)), run(k=9, flip=False)], cells=(0.25,), exact_plane=True),
    ]
    return cs


def cases():
    return {c["name"]: c for c in all_cases()}


def surface_of(case):
    return case["cloud"] if case["surface"] is None else case["surface"]


@functools.lru_cache(maxsize=None)
def ref(name, i):
    """the reference of run i of a case, computed once and shared by the tests that need it (never modified)"""
    import normal_reference as nr
    c = cases()[name]
    r = c["runs"][i]
    return nr.estimate(c["cloud"], c["surface"], k=r["k"], radius=r["radius"], viewpoint=r["vp"], flip=r["flip"])
