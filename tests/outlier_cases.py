"""Designed clouds for the outlier filters (rgc_outlier_*): every case is dict(name, cloud (n, 3) float32, sor, ror, cells, minima) -- sor: (mean_k, std_mul)
pairs of StatisticalOutlierRemoval, ror: (radius, min_neighbors) pairs of RadiusOutlierRemoval, cells: explicit cell sizes of the filters' grid tried
beside the automatic rule, minima: what the REFERENCE ALONE proves the case contains (tests/test_outlier_reference.py checks them on the CPU, together
with the rule every SOR setting obeys: NO mean distance lies within the derived bound of the reference threshold, outlier_reference.sor()['undecided']
== 0 -- std_mul is chosen per case so that this holds).  The GPU tests (tests/test_gpu_outlier.py) compare the product with the reference on every point.

  lattice     8 x 8 x 8 points at spacing 2^-3 m about (100, -60, 2): every key is exact, neighbours tie exactly.  ROR at radius = the spacing exactly
              (the six face neighbours lie ON the radius: excluded, count = 1 everywhere), at the next double above it (float32(r r) is the same r2: still
              1), and at 0.13 (corners 4, edges 5, faces 6, interior 7) with min_neighbors = 5: count - 1 == 5 and == 4 both occur
  dups        64 points, each three times: ranks 1 and 2 of every row are duplicates at key 0, like rank 0
  strays      a 2 000-point sheet and 20 strays 50 to 500 m away: their cubes grow to the whole grid; every stray is removed at std_mul = 1, and has
              count = 1 under ROR
  line        collinear points (the grid is one row of cells along a diagonal)
  pair        n = 2 with mean_k = 1: both mean distances equal the threshold EXACTLY (outlier_reference's exact case): both kept, none with negative
  full_K      n = mean_k + 1 at mean_k + 1 = 4, 5, 8, 9, 16, 17, 32, 33, 64: both sides of every list tier, every row the whole cloud
  n_N         n = 255 / 256 / 257 and 2047 / 2048 / 2049: workgroup and scan-block seams
  mid         1 500 points at mean_k = 3, 20 and 50 (tiers 4, 32, 64 with more candidates than entries)
  big         70 001 points: 274 rows of partial sums, more than one pass of the 64-lane fold"""
import functools

import numpy as np

CENTER = np.array([100.0, -60.0, 2.0])
SPACING = 0.125
FULL_K = (4, 5, 8, 9, 16, 17, 32, 33, 64)
SEAM_N = (255, 256, 257, 2047, 2048, 2049)


def _box(rng, n, ext):
    return (rng.uniform(-1, 1, (n, 3)) * np.asarray(ext) + CENTER).astype(np.float32)


@functools.lru_cache(maxsize=None)
def lattice_case():
    rng = np.random.default_rng(2201)
    I = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3)
    I = I[rng.permutation(len(I))]
    cloud = (I * SPACING + CENTER).astype(np.float32)      # exact: 100 + i / 8
    return dict(name="lattice", cloud=cloud, sor=((6, 1.0), (26, 0.5)), ror=((SPACING, 0), (float(np.nextafter(SPACING, 1.0)), 0), (0.13, 5)), cells=(0.25, 4.0),
                minima=dict(count_1={SPACING: 512, float(np.nextafter(SPACING, 1.0)): 512}, on_gate={0.13: (5, 216, 72)}, tied_rows=512))


@functools.lru_cache(maxsize=None)
def dups_case():
    rng = np.random.default_rng(2202)
    base = _box(rng, 64, (2, 2, 0.5))
    cloud = np.repeat(base, 3, axis=0)[rng.permutation(192)]
    return dict(name="dups", cloud=cloud, sor=((5, 1.0), (2, 1.0)), ror=((0.4, 3),), cells=(0.25, 4.0), minima=dict(zero_ranks=2))


@functools.lru_cache(maxsize=None)
def strays_case():
    rng = np.random.default_rng(2203)
    sheet = np.concatenate([rng.uniform(-5, 5, (2000, 2)), rng.normal(0, 0.01, (2000, 1))], axis=1)
    ang = np.arange(20) * (2 * np.pi / 20)
    rad = np.linspace(50.0, 500.0, 20)
    strays = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.linspace(-20, 20, 20)], axis=1)
    cloud = (np.concatenate([sheet, strays]) + CENTER).astype(np.float32)
    perm = rng.permutation(len(cloud))
    return dict(name="strays", cloud=cloud[perm], sor=((8, 1.0),), ror=((1.0, 2),), cells=(4.0,), strays=np.flatnonzero(perm >= 2000).astype(np.int32),
                minima=dict(strays_removed=20, stray_count_1=20))


@functools.lru_cache(maxsize=None)
def line_case():
    rng = np.random.default_rng(2204)
    t = np.sort(rng.uniform(-20, 20, 300))
    cloud = (t[:, None] * np.array([[0.6, 0.48, 0.64]]) + CENTER).astype(np.float32)
    return dict(name="line", cloud=cloud[rng.permutation(300)], sor=((4, 1.0),), ror=((0.3, 3),), cells=(0.25, 4.0), minima=dict())


@functools.lru_cache(maxsize=None)
def pair_case():
    cloud = (np.array([[0.0, 0.0, 0.0], [0.3, -0.2, 0.1]]) + CENTER).astype(np.float32)
    return dict(name="pair", cloud=cloud, sor=((1, 1.0),), ror=((0.5, 1), (0.1, 1)), cells=(0.25, 4.0), minima=dict(exact=True))


@functools.lru_cache(maxsize=None)
def full_case(k1):
    rng = np.random.default_rng(2210 + k1)
    return dict(name="full_%d" % k1, cloud=_box(rng, k1, (1, 1, 1)), sor=((k1 - 1, 1.0),), ror=((0.7, 2),), cells=(0.25,), minima=dict())


@functools.lru_cache(maxsize=None)
def seam_case(n):
    rng = np.random.default_rng(2300 + n)
    return dict(name="n_%d" % n, cloud=_box(rng, n, (4, 4, 1)), sor=((8, 1.0),), ror=((0.5, 4),), cells=(), minima=dict())


@functools.lru_cache(maxsize=None)
def mid_case():
    rng = np.random.default_rng(2205)
    return dict(name="mid", cloud=_box(rng, 1500, (3, 3, 1)), sor=((3, 1.0), (20, 1.5), (50, 2.0)), ror=((0.4, 6),), cells=(0.25, 4.0), minima=dict())


@functools.lru_cache(maxsize=None)
def big_case():
    rng = np.random.default_rng(2206)
    return dict(name="big", cloud=_box(rng, 70001, (20, 20, 2)), sor=((8, 1.0),), ror=((0.5, 5),), cells=(), minima=dict(stat_rows=274))


def small_cases():
    """the cases the brute force pins the reference on"""
    return [lattice_case(), dups_case(), line_case(), pair_case(), mid_case()] + [full_case(k) for k in FULL_K] + [seam_case(n) for n in SEAM_N[:3]]


def all_cases():
    return [lattice_case(), dups_case(), strays_case(), line_case(), pair_case(), mid_case(), big_case()] + [full_case(k) for k in FULL_K] + [seam_case(n) for n in SEAM_N]


# ---- the reference of a case, computed once per setting and shared by the tests that need it (never modified) ----
CASES = {c["name"]: c for c in all_cases()}


@functools.lru_cache(maxsize=None)
def ref_sor(name, mean_k, std_mul):
    import outlier_reference as orf
    return orf.sor(CASES[name]["cloud"], mean_k, std_mul)


@functools.lru_cache(maxsize=None)
def ref_counts(name, radius):
    import outlier_reference as orf
    return orf.counts(CASES[name]["cloud"], radius)
