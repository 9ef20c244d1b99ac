"""Designed clouds for Euclidean cluster extraction (rgc_cluster_extract): every case is dict(name, cloud (n, 3) float32, tol, limits, minima, small) --
tol: the tolerances it is run at, limits: (min_size, max_size) pairs, minima: what the REFERENCE ALONE proves the case contains at (tol[0], limits[0])
(tests/test_cluster_reference.py checks them on the CPU), small: the literal restatement of PCL's algorithm is run on it too.  The GPU tests
(tests/test_gpu_cluster.py) compare the product with the reference for equality.

Where a threshold must be exact the coordinates are dyadic (multiples of 2^-6 m) and the tolerance is 0.5, so r2 = 0.25 exactly and every key is exact.

  thr_origin / thr_wall / thr_far   pairs 8 m apart: at distance exactly 0.5 along x, y and z (key == r2: two clusters each), one fp32 step of the
              coordinate inside (one cluster), duplicates (one cluster); at the origin also a pair whose key is exactly one fp32 step under r2.  _wall: the
              pairs moved so that they straddle the walls at x = 2 of cells of 1/16, 0.5 and 4 m; _far: 1000 m from the origin
  chain_N / iso_N   N = 1, 2, 63, 64, 65, 255, 256, 257 points on a line at spacing 0.375 (one cluster) / 0.5 (N clusters of one point)
  helix_N_ORDER   N = 3, 65, 257, 4097, 20000 points at 0.375 along a square spiral that rises 2^-5 per step (2 m per turn: three extents, no two
              turns within reach); input index ascending along the chain, descending, shuffled -- the union-find's worst case, a path
  helix_gap   a 257-chain with one step of exactly 0.5 whose middle lies on the cell wall x = 1.75 (cells of 0.5): two clusters
  helix_dup3  the 20 000-chain, every point three times
  double_helix  two interleaved 256-point spirals (one turned by 180 degrees) that never come closer than 1 - 2^-5 > 0.5 + 2^-6: two clusters of equal
              size with identical bounding boxes
  lattice_T   17 x 17 x 17 points at spacing 0.5 at tolerance 0.5 (every point isolated: 4913 clusters of size 1, every order decided by the leader),
              0.5 + 2^-6 and 0.8 (between 0.5 sqrt 2 and 0.5 sqrt 3): one component
  limits      components of sizes 1 .. 8, six copies of each, input shuffled; (min_size, max_size) = (1, INT_MAX), (3, 3), (2, 7), (8, 8) and (9, 100)
              (nothing kept): a component over max_size is dropped whole; the six-fold ties are ordered by leader
  copies / ball   5 000 copies of one point / 5 000 points in a ball of radius 0.1: everything in one cell, one cluster
  blobs_N     Gaussian blobs plus uniform noise, N = 2 000 and 30 000, at three tolerances; scan: one synthetic LiDAR scan"""
import functools

import numpy as np

INT_MAX = 2 ** 31 - 1
STEP = 0.375
SIZES_N = (1, 2, 63, 64, 65, 255, 256, 257)
HELIX_N = (3, 65, 257, 4097, 20000)
LIMITS = ((1, INT_MAX), (3, 3), (2, 7), (8, 8), (9, 100))


def _case(name, cloud, tol=(0.5,), limits=((1, INT_MAX),), minima=None, small=True):
    raw = np.asarray(cloud)
    cloud = np.ascontiguousarray(raw, np.float32)
    assert np.array_equal(cloud.astype(np.float64), raw.astype(np.float64)), "every designed coordinate is a float32"
    return dict(name=name, cloud=cloud, tol=tuple(tol), limits=tuple(limits), minima=minima or {}, small=small)


def _threshold(name, o, with_one_under):
    o = np.asarray(o, np.float64)
    rows = []
    f32 = lambda v: np.float32(v)
    def pair(k, a, b):
        base = o + np.array([0.0, 8.0 * k, 0.0])
        rows.append(base + a)
        rows.append(base + b)
    z = np.zeros(3)
    for k, axis in enumerate(range(3)):                         # exactly 0.5 apart along each axis: key == r2, not joined
        d = np.zeros(3)
        d[axis] = 0.5
        pair(k, z, d)
    cloud = [np.asarray(r, np.float64) for r in rows]
    # one fp32 step of the coordinate inside: joined
    a = o + np.array([0.0, 24.0, 0.0])
    b = a.copy()
    b[0] = float(np.nextafter(f32(a[0] + 0.5), f32(a[0])))
    cloud += [a, b]
    a = o + np.array([0.0, 32.0, 0.0])                           # duplicates
    cloud += [a, a.copy(), a.copy()]
    if with_one_under:                                           # (0.5 - 2^-25)^2 rounds to 0.25 - 2^-25; + (2^-13)^2 = 0.25 - 2^-26: one step under r2
        a = np.array([0.0, 40.0, 0.0])
        cloud += [a, a + np.array([0.5 - 2.0 ** -25, 2.0 ** -13, 0.0])]
    cloud = np.array(cloud)
    rng = np.random.default_rng(2301)
    cloud = cloud[rng.permutation(len(cloud))]
    minima = dict(n_clusters=8 + (1 if with_one_under else 0), at_r2=3, ties=6, one_under=1 if with_one_under else 0)
    return _case(name, cloud, minima=minima)


def _spiral(n, gap_at=None):
    """n points of a square spiral of side 16 steps in x, y, rising 2^-5 per step; gap_at: the step from point gap_at to the next is exactly 0.5 along x, level"""
    p = np.zeros((n, 3))
    pos = np.zeros(3)
    dirs = ((1, 0), (0, 1), (-1, 0), (0, -1))
    for i in range(n):
        p[i] = pos
        d = dirs[(i // 16) % 4]
        if gap_at is not None and i == gap_at:
            pos = pos + np.array([0.5, 0.0, 0.0])
        else:
            pos = pos + np.array([d[0] * STEP, d[1] * STEP, 2.0 ** -5])
    return p


def _ordered(p, order, seed):
    if order == "asc":
        return p
    if order == "desc":
        return p[::-1]
    return p[np.random.default_rng(seed).permutation(len(p))]


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = [_threshold("thr_origin", (0.0, 0.0, 0.0), True), _threshold("thr_wall", (1.75, 0.0, 0.0), False), _threshold("thr_far", (1000.0, -1000.0, 1000.0), False)]
    for n in SIZES_N:
        x = np.arange(n)[:, None]
        cases.append(_case("chain_%d" % n, x * np.array([[STEP, 0, 0]]) + np.array([[3.0, 1.0, -2.0]]), minima=dict(n_clusters=1, largest=n)))
        cases.append(_case("iso_%d" % n, x * np.array([[0.5, 0, 0]]) + np.array([[3.0, 1.0, -2.0]]), minima=dict(n_clusters=n, at_r2=n - 1, ties=n if n > 1 else 0)))
    for n in HELIX_N:
        for order in ("asc", "desc", "shuf"):
            cases.append(_case("helix_%d_%s" % (n, order), _ordered(_spiral(n), order, 2400 + n), minima=dict(n_clusters=1, largest=n), small=n <= 4097 and order == "asc"))
    cases.append(_case("helix_gap", _ordered(_spiral(257, gap_at=4), "shuf", 2411), minima=dict(n_clusters=2, at_r2=1, largest=252)))
    dup = np.repeat(_spiral(20000), 3, axis=0)
    cases.append(_case("helix_dup3", _ordered(dup, "shuf", 2412), minima=dict(n_clusters=1, largest=60000), small=False))
    a = _spiral(256)
    b = a.copy()
    b[:, 0], b[:, 1] = 6.0 - a[:, 0], 6.0 - a[:, 1]              # the spiral's square is [0, 6]^2: turned by 180 degrees about its middle
    cases.append(_case("double_helix", _ordered(np.concatenate([a, b]), "shuf", 2413), tol=(0.5, 0.5 + 2.0 ** -6), minima=dict(n_clusters=2, ties=2, largest=256)))
    I = np.stack(np.meshgrid(np.arange(17), np.arange(17), np.arange(17), indexing="ij"), axis=-1).reshape(-1, 3)
    I = I[np.random.default_rng(2414).permutation(len(I))]
    lat = I * 0.5 + np.array([[-20.0, 7.0, 1.5]])
    cases.append(_case("lattice_iso", lat, tol=(0.5,), minima=dict(n_clusters=4913, ties=4913, at_r2=3 * 17 * 17 * 16)))
    cases.append(_case("lattice_one", lat, tol=(0.5 + 2.0 ** -6, 0.8), minima=dict(n_clusters=1, largest=4913)))
    comps = []
    for size in range(1, 9):
        for copy in range(6):
            comps.append(np.arange(size)[:, None] * np.array([[STEP, 0, 0]]) + np.array([[0.0, 5.0 * copy, 5.0 * size]]))
    lim = np.concatenate(comps)
    lim = lim[np.random.default_rng(2415).permutation(len(lim))]
    cases.append(_case("limits", lim, limits=LIMITS, minima=dict(n_clusters=48, ties=48)))
    rng = np.random.default_rng(2416)
    cases.append(_case("copies", np.tile(np.array([[12.5, -3.25, 0.75]]), (5000, 1)), minima=dict(n_clusters=1, largest=5000), small=False))
    v = rng.normal(size=(5000, 3))
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * (0.1 * rng.uniform(0, 1, (5000, 1)) ** (1 / 3))
    cases.append(_case("ball", (v + np.array([[12.5, -3.25, 0.75]])).astype(np.float32), tol=(0.5, 0.02), minima=dict(n_clusters=1, largest=5000), small=False))
    return cases


def _blobs(n, seed):
    rng = np.random.default_rng(seed)
    nb = n * 3 // 4
    centres = rng.uniform(-30, 30, (40, 3)) * np.array([1, 1, 0.1])
    pts = centres[rng.integers(0, 40, nb)] + rng.normal(0, 0.6, (nb, 3))
    noise = rng.uniform(-35, 35, (n - nb, 3)) * np.array([1, 1, 0.15])
    return np.concatenate([pts, noise])[rng.permutation(n)].astype(np.float32)


@functools.lru_cache(maxsize=None)
def general_cases():
    from rgc_slam_amd import synth
    world, _ = synth.make_world_and_map(30000)
    scan = np.ascontiguousarray(synth.make_scan_n(world, np.eye(4), 8000)["xyz"], np.float32)
    return [_case("blobs_2000", _blobs(2000, 2420), tol=(0.2, 0.5, 1.0), limits=((1, INT_MAX), (5, 400)), small=False),
            _case("blobs_30000", _blobs(30000, 2421), tol=(0.2, 0.5, 1.0), limits=((1, INT_MAX), (5, 4000)), small=False),
            _case("scan", scan, tol=(0.2, 0.5, 1.0), limits=((1, INT_MAX), (10, 2000)), small=False)]


CASES = {c["name"]: c for c in all_cases()}


def case(name):
    return CASES[name] if name in CASES else {c["name"]: c for c in general_cases()}[name]


# ---- the reference of a case, computed once per setting and shared by the tests that need it (never modified) ----
@functools.lru_cache(maxsize=None)
def ref(name, tol, min_size=1, max_size=INT_MAX):
    import cluster_reference as cr
    return cr.extract(case(name)["cloud"], tol, min_size, max_size)
