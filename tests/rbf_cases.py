"""The clouds tests/test_rbf_reference.py and tests/test_gpu_rbf.py share: name -> (points (n, 3) float32, kernel_width, max_dist, voxel_res), and the
reference's moments of each, computed once (``mom``).  Small on purpose: each is the smallest cloud at which the kernel can still go wrong."""
import functools

import numpy as np

import rbf_reference as rr

SPACING = 0.25          # the dyadic lattice: 17^3 points, max_dist = 1 = 4 spacings: i^2 + j^2 + k^2 <= 16 has 257 solutions, 6 of them with = 16
LATTICE_N = 17


def _lattice():
    g = np.arange(LATTICE_N, dtype=np.float32) * np.float32(SPACING)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return P[np.random.default_rng(5).permutation(len(P))].copy()


def lattice_interior(P):
    i = np.rint(P / SPACING).astype(int)
    return np.all((i >= 4) & (i <= LATTICE_N - 5), axis=1)


def _knife():
    """res = 1, max_dist = 3.  The issue's pair: x = nextafter(1, 0) and x = 4 (dx rounds to 3.0f, the key to 9.0f = max_dist_sq), and the same pair moved
    onto the grid's walls (cells are [(c + 0.5) res, (c + 1.5) res)): x = nextafter(1.5, 0) in cell 0 and x = 4.5 in cell 4, a member at a cell offset of 4."""
    rng = np.random.default_rng(6)
    bg = rng.uniform(0.0, 6.0, (300, 3)).astype(np.float32)
    pairs = np.array([[np.nextafter(np.float32(1.0), np.float32(0.0)), 0.75, 0.75], [4.0, 0.75, 0.75],
                      [np.nextafter(np.float32(1.5), np.float32(0.0)), 2.25, 5.25], [4.5, 2.25, 5.25]], np.float32)
    return np.concatenate([pairs, bg])


def _crowded():
    """one cell of a 1 m grid with 400 points (more than a candidate tile of 256 and than a workgroup's run of 64) among sparse neighbours"""
    rng = np.random.default_rng(7)
    cell = (np.float32([2.5, 2.5, 2.5]) + rng.uniform(0.02, 0.98, (400, 3))).astype(np.float32)
    bg = rng.uniform(0.0, 6.0, (500, 3)).astype(np.float32)
    P = np.concatenate([cell, bg])
    return P[rng.permutation(len(P))].copy()


def _scene(n_floor=40, seed=8):
    """a jittered floor (10 m x 10 m at 0.25 m) and a wall on it, at map-like coordinates"""
    rng = np.random.default_rng(seed)
    u = np.arange(n_floor) * 0.25
    fx, fy = np.meshgrid(u, u, indexing="ij")
    floor = np.stack([fx.ravel(), fy.ravel(), np.zeros(fx.size)], axis=1)
    wy, wz = np.meshgrid(u, np.arange(1, 16) * 0.25, indexing="ij")
    wall = np.stack([np.full(wy.size, 6.0), wy.ravel(), wz.ravel()], axis=1)
    P = np.concatenate([floor, wall]) + rng.normal(0.0, 0.03, (fx.size + wy.size, 3)) + np.array([412.0, -187.0, 12.0])
    return P.astype(np.float32)


def _tiny(n):
    return np.random.default_rng(100 + n).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)


def _isolated():
    P = np.random.default_rng(9).uniform(0.0, 3.0, (200, 3)).astype(np.float32)
    P[17] = (40.0, -35.0, 20.0)
    return P


ISOLATED_ROW = 17


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(11)
    if name.startswith("lattice"):                       # lattice_0.5, lattice_1, lattice_2: reach 3, 2 and 1 cells, max_dist a multiple of res
        return _lattice(), 1.0, 1.0, float(name.split("_")[1])
    if name == "knife":
        return _knife(), 0.5, 3.0, 1.0
    if name == "short":                                  # max_dist < res
        return rng.uniform(0.0, 8.0, (1500, 3)).astype(np.float32), 2.0, 0.7, 2.0
    if name == "all_pairs":                              # max_dist larger than the cloud: every pair is a member
        return rng.uniform(-2.0, 2.0, (700, 3)).astype(np.float32), 0.05, 100.0, 1.0
    if name == "corners":                                # a 4^3-cell box filled to its corners: every clamp of the rows' and spans' ends
        return rng.uniform(0.5, 4.5, (600, 3)).astype(np.float32), 0.5, 1.5, 1.0
    if name == "crowded":
        return _crowded(), 1.0, 1.2, 1.0
    if name.startswith("tiny_"):
        return _tiny(int(name.split("_")[1])), 0.5, 3.0, 1.0
    if name == "isolated":
        return _isolated(), 0.5, 3.0, 1.0
    if name == "scene":                                  # the defaults 0.5 / 3.0
        return _scene(), 0.5, 3.0, 1.0
    if name == "scene_src":
        return _scene(24, seed=12), 0.5, 3.0, 1.0
    raise KeyError(name)


NONE_CASES = ["lattice_0.5", "lattice_1", "lattice_2", "knife", "short", "all_pairs", "corners", "crowded", "tiny_1", "tiny_2", "tiny_63", "tiny_64", "tiny_65",
              "isolated", "scene"]
# generic jittered clouds with full balls.  NONE only: the lattice (its moments are isotropic) and the clouds whose balls hold one or two points
# ("short", the tiny ones, "isolated": moments of rank 0 and 1, no eigenvector to compare)
EIGEN_CASES = ["scene", "corners", "crowded"]


@functools.lru_cache(maxsize=None)
def mom(name):
    P, kw, md, _ = case(name)
    return rr.moments(P, kw, md)
