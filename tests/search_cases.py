"""Designed inputs for the search index (rgc_search_*): every case is dict(name, tgt, qry, ks, radii, cells, minima[, grow]) -- ks: the k values of
nearestKSearch, radii: (r, max_nn) pairs of radiusSearch, cells: explicit cell sizes (0 = the automatic rule is always tried too), minima: lower bounds
of search_reference.census met by the REFERENCE ALONE (tests/test_search_reference.py checks that on the CPU), grow: (k, cell, least queries whose
cube must grow).  The GPU tests (tests/test_gpu_search.py) compare the product with the reference on every query of every case.

  lattice     coordinates on the 2^-6 m lattice about (100, -60, 2): every key is exact in fp32, so ties at the k-th place, ties at the max_nn cut and
              members ON the gate (key == r2, excluded) are exact.  Queries on the lattice, some equal to indexed points, some outside the box
  dups        40 copies of one point (more than any k) among 200 others: a row of equal keys is ordered by index alone
  sheet       a plane z = const (the grid has one layer); line: y = z = const (one row of cells)
  sparse      300 points in a 200 m box at 1 m cells: the cube grows three times and more
  dense_cell  3000 points inside one 1 m cell
  tiny_*      targets of 1, 2, 4, 5, 6, 31, 32 points: rows shorter than k, k = n and k = n + 1
  walls       nn_cases.wall_ulp_case: indexed points within one fp32 ulp of a cell wall, queries across it, and queries ON the walls
  far         queries 1e6 m outside the box
  window      balls of window - 1, window, window + 1 and 1.2 x window members (the sort's long route), 1 and 0 members; whole: r takes in the cloud"""
import functools

import numpy as np

import nn_cases
import nn_reference as nn

ALL_K = (1, 2, 5, 8, 9, 16, 17, 31, 32)
CENTER = np.array([100.0, -60.0, 2.0])
DEFAULT_WINDOW = 4096   # rgc_search_sort_window() of the library as built (tests/test_search_api.py holds the two together)
NQ_COUNTS = (1, 63, 64, 65, 100)   # 100: no multiple of a workgroup's queries (64 at four lanes per query, 32 at eight)


def _lat(I):
    return (nn.lattice(I).astype(np.float64) + CENTER).astype(np.float32)   # exact: 100 + i / 64 has 13 significant bits


@functools.lru_cache(maxsize=None)
def lattice_case():
    rng = np.random.default_rng(2101)
    It = np.unique(rng.integers(-40, 41, (6500, 3)), axis=0)
    It = It[rng.permutation(len(It))]
    Iq = np.concatenate([rng.integers(-44, 45, (1300, 3)), It[rng.integers(0, len(It), 300)], rng.integers(41, 60, (60, 3))])
    return dict(name="lattice", tgt=_lat(It), qry=_lat(Iq), ks=ALL_K, radii=((0.125, 0), (0.125, 1), (0.125, 5), (0.125, 32), (0.0625, 0)),
                cells=(0.0625, 0.25, 1.0), minima=dict(knn_tie=2000, maxnn_tie=300, on_r2=300, on_point=300, outside=60, rows_0=50, rows_small=1000),
                grow=(32, 0.0625, 1000))


@functools.lru_cache(maxsize=None)
def dups_case():
    rng = np.random.default_rng(2102)
    Io = np.unique(rng.integers(-30, 31, (200, 3)), axis=0)
    It = np.concatenate([np.tile([[3, -2, 5]], (40, 1)), Io])
    It = It[rng.permutation(len(It))]
    Iq = np.concatenate([[[3, -2, 5], [4, -2, 5], [3, -2, 4]], rng.integers(-30, 31, (97, 3))])
    return dict(name="dups", tgt=_lat(It), qry=_lat(Iq), ks=ALL_K, radii=((0.05, 0), (0.05, 5), (0.05, 32)), cells=(0.25,),
                minima=dict(knn_tie=9, maxnn_tie=2, on_point=1))


@functools.lru_cache(maxsize=None)
def sheet_case():
    rng = np.random.default_rng(2103)
    t = np.concatenate([rng.uniform(-10, 10, (5000, 2)), np.full((5000, 1), 1.25)], axis=1).astype(np.float32)
    q = np.concatenate([rng.uniform(-11, 11, (900, 2)), rng.normal(1.25, 0.5, (900, 1))], axis=1).astype(np.float32)
    return dict(name="sheet", tgt=t, qry=q, ks=(1, 5, 17, 32), radii=((0.5, 0), (0.5, 5)), cells=(0.5, 2.0), minima=dict(outside=100, rows_small=300))


@functools.lru_cache(maxsize=None)
def line_case():
    rng = np.random.default_rng(2104)
    t = np.stack([rng.uniform(-50, 50, 2000), np.full(2000, -3.0), np.full(2000, 0.5)], axis=1).astype(np.float32)
    q = np.stack([rng.uniform(-55, 55, 400), rng.normal(-3.0, 0.3, 400), rng.normal(0.5, 0.3, 400)], axis=1).astype(np.float32)
    return dict(name="line", tgt=t, qry=q, ks=(1, 5, 9, 32), radii=((0.4, 0), (0.4, 1)), cells=(0.5, 4.0), minima=dict(outside=300, rows_0=20, rows_small=100))


@functools.lru_cache(maxsize=None)
def sparse_case():
    rng = np.random.default_rng(2105)
    t = rng.uniform(-100, 100, (300, 3)).astype(np.float32)
    q = rng.uniform(-100, 100, (257, 3)).astype(np.float32)
    return dict(name="sparse", tgt=t, qry=q, ks=(1, 5, 16, 32), radii=((30.0, 0), (30.0, 5)), cells=(1.0, 4.0), minima=dict(rows_small=100),
                grow=(5, 1.0, 200))


@functools.lru_cache(maxsize=None)
def dense_cell_case():
    rng = np.random.default_rng(2106)
    t = np.concatenate([rng.uniform(0.55, 1.45, (3000, 3)), rng.uniform(-10, 10, (50, 3))]).astype(np.float32)   # cell 0 of a 1 m grid is [0.5, 1.5)
    q = np.concatenate([rng.uniform(0.4, 1.6, (180, 3)), rng.uniform(-10, 10, (20, 3))]).astype(np.float32)
    return dict(name="dense_cell", tgt=t, qry=q, ks=(1, 8, 31, 32), radii=((0.2, 0), (0.2, 32), (0.2, 1)), cells=(1.0,), minima=dict(rows_small=150))


def tiny_case(n):
    rng = np.random.default_rng(2200 + n)
    t = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    q = rng.uniform(-3, 3, (65, 3)).astype(np.float32)
    ks = (1, 2, 5, 32)
    return dict(name="tiny_%d" % n, tgt=t, qry=q, ks=ks, radii=((2.0, 0), (2.0, 5), (100.0, 0)), cells=(0.5,),
                minima=dict(short_rows=65 * sum(k > n for k in ks), rows_whole=65))


TINY_N = (1, 2, 4, 5, 6, 31, 32)


@functools.lru_cache(maxsize=None)
def walls_case():
    res = 0.5
    t, s = nn_cases.wall_ulp_case(res)
    on_wall = t[:300].copy()
    on_wall[:, 0] = ((np.floor(on_wall[:, 0].astype(np.float64) / res - 0.5) + 0.5) * res).astype(np.float32)   # exactly on the cell's lower wall
    q = np.concatenate([s, on_wall, np.nextafter(on_wall, np.float32(np.inf)), np.nextafter(on_wall, np.float32(-np.inf))]).astype(np.float32)
    return dict(name="walls", tgt=t, qry=q, ks=(1, 2, 5), radii=((0.13, 0), (0.13, 1)), cells=(0.5,), minima=dict(rows_1=3000, rows_0=100, outside=100))


@functools.lru_cache(maxsize=None)
def far_case():
    rng = np.random.default_rng(2107)
    t = _lat(np.unique(rng.integers(-30, 31, (2000, 3)), axis=0))
    far = np.array([[1e6, 0, 0], [-1e6, 0, 0], [0, 1e6, 0], [0, 0, -1e6], [1e6, 1e6, 1e6], [-1e6, 1e6, -1e6]], np.float64) + CENTER
    q = np.concatenate([far.astype(np.float32), t[:10]])
    return dict(name="far", tgt=t, qry=q, ks=(1, 5, 32), radii=((0.5, 0), (0.5, 5)), cells=(0.125, 1.0), minima=dict(outside=6, rows_0=6))


@functools.lru_cache(maxsize=None)
def window_case(window=DEFAULT_WINDOW):
    """six balls of radius 0.4 about centres 10 m apart holding window - 1, window, window + 1, 1.2 x window, 1 and 0 points; r = 0.5 about each centre
    takes in exactly its ball"""
    rng = np.random.default_rng(2108)
    sizes = (window - 1, window, window + 1, window + window // 5, 1, 0)
    pts, ctr = [], []
    for j, m in enumerate(sizes):
        c = np.array([10.0 * j, 3.0, -1.0])
        d = rng.normal(size=(m, 3))
        d *= (0.4 * rng.uniform(0, 1, (m, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
        pts.append(c + d)
        ctr.append(c)
    t = np.concatenate(pts).astype(np.float32)
    t = t[rng.permutation(len(t))]
    return dict(name="window", tgt=t, qry=np.asarray(ctr, np.float32), ks=(32,), radii=((0.5, 0), (0.5, 32)), cells=(0.25,), window=window,
                minima=dict(rows_0=1, rows_1=1, rows_window_m1=1, rows_window=1, rows_window_p1=1, rows_long=2))


@functools.lru_cache(maxsize=None)
def whole_case():
    rng = np.random.default_rng(2109)
    t = rng.uniform(-5, 5, (577, 3)).astype(np.float32)
    q = rng.uniform(-5, 5, (33, 3)).astype(np.float32)
    return dict(name="whole", tgt=t, qry=q, ks=(9,), radii=((40.0, 0), (40.0, 32)), cells=(1.0,), minima=dict(rows_whole=33))


def small_cases():
    """the cases the brute force pins the wrappers on (a few hundred thousand pairs each)"""
    return [dups_case(), sparse_case(), whole_case(), far_case()] + [tiny_case(n) for n in TINY_N]


def all_cases():
    return [lattice_case(), dups_case(), sheet_case(), line_case(), sparse_case(), dense_cell_case(), walls_case(), far_case(), window_case(), whole_case()] + [
        tiny_case(n) for n in TINY_N]
