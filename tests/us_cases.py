"""Inputs of the UniformSampling / keyframe-selection tests (tests/test_us_reference.py on the CPU, tests/test_gpu_uniform_sampling.py and
tests/test_gpu_kf_select.py on the GPU), each with the MINIMA its census must reach -- the census is computed from tests/us_reference.py alone, so a
case that no longer exercises what it is for fails without a GPU."""
import numpy as np

import pre_cases as pc
import us_reference as us

F = np.float32


# ---- clouds for rgc_uniform_sampling -----------------------------------------------------------------------------------------------------
def lattice(n=3000, seed=71):
    """coordinates k / 16 (every product, difference and square below is exact in fp32: ties are EXACT ties), negative ones included; leaf 0.5 puts the
    leaf centres on the lattice, so points mirrored about a centre tie"""
    rng = np.random.default_rng(seed)
    k = np.stack([rng.integers(-96, 96, n), rng.integers(-96, 96, n), rng.integers(-32, 32, n)], axis=1)
    out = np.empty((n, 4), F)
    out[:, :3] = k.astype(F) / F(16)
    out[:, 3] = rng.integers(0, 64, n) + rng.random(n).astype(F)
    return out


LATTICE_MINIMA = dict(leaves=1500, tie_leaves=20, winner_not_first=100)

LEAF_POPULATIONS = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 6000)


def big_leaves(plant, seed=72, leaf=0.5, spread=False):
    """one leaf per population of LEAF_POPULATIONS (the filter's workgroup size, its scan block and the bucket sizes of test_gpu_pre_routes.py, either side),
    strung along x with gaps, negative leaf coordinates included, in shuffled point order.  Every member lies more than 0.2 leaf from its leaf's centre but
    ONE, the planted winner, at member rank (ascending input index)
        plant = "first": 0, and a copy of its coordinates as the LAST member (an exact tie the first must win);
        plant = "last": population - 1;
        plant = "boundary": b - 1 for the largest b of 64, 256, 2048, 4096 below the population (else the middle), with a copy of its coordinates at rank b:
                an exact tie across the boundary slot, which the lower index must win.
    spread: two more points 300 leaves out in y and 50 in z, so that the grid is sparse (the sort's buckets are whole rows, the fullest over 4095 points)
    instead of dense (leaf buckets).
    -> (cloud (n, 4), planted (len(LEAF_POPULATIONS),) input indices of the winners, in ascending leaf index)"""
    rng = np.random.default_rng(seed)
    pops = np.array(LEAF_POPULATIONS)
    n = int(pops.sum())
    label = np.repeat(np.arange(len(pops)), pops)[rng.permutation(n)]
    out = np.empty((n, 4), F)
    out[:, 3] = rng.random(n).astype(F) * 100
    planted = np.zeros(len(pops), np.int64)
    for j, pop in enumerate(pops):
        mem = np.flatnonzero(label == j)
        ijk = np.array([3 * j - 20, (j % 3) - 1, -1], np.float64)
        u = rng.uniform(0.03, 0.97, (pop, 3))
        near = np.abs(u - 0.5).max(axis=1) < 0.2
        u[near, 0] = 0.1 + 0.1 * rng.random(int(near.sum()))
        out[mem, :3] = ((ijk + u) * leaf).astype(F)
        if plant == "first":
            r, copy = 0, pop - 1
        elif plant == "last":
            r, copy = pop - 1, None
        else:
            b = [x for x in (64, 256, 2048, 4096) if x < pop]
            r = b[-1] - 1 if b else pop // 2
            copy = r + 1
        out[mem[r], :3] = ((ijk + [0.51, 0.495, 0.5]) * leaf).astype(F)
        if copy is not None and copy != r and copy < pop:
            out[mem[copy], :3] = out[mem[r], :3]
        planted[j] = mem[r]
    if spread:
        far = np.array([[0.1, 300.2 * leaf, 50.3 * leaf, 1.0], [0.1, -299.7 * leaf, -49.6 * leaf, 2.0]], F)
        out = np.ascontiguousarray(np.concatenate([out, far]))
    return out, planted


def walls(leaf, seed=73):
    """points ON the leaf walls fp32(m * leaf), their fp32 neighbours either side and their mirror images (pre_cases.wall_points): which leaf a point falls
    into is decided by the rounding of p * inv"""
    return pc.wall_points(leaf, seed)


def rounding_decides(xyz, leaf):
    """number of coordinates whose leaf under the fp32 product differs from the leaf of the exact quotient p / leaf"""
    p = np.asarray(xyz, F)[:, :3]
    exact = np.floor(p.astype(np.float64) / np.float64(F(leaf))).astype(np.int64)
    return int((us.pr.leaf_coords(p, leaf) != exact).sum())


# ---- key poses for the selections --------------------------------------------------------------------------------------------------------
def lattice_drive(n, seed=74):
    """n key poses of a serpentine drive on the lattice 1/16 + k/8 (rows of 100, 1/8 m apart; z on k/16): at leaf 0.5 every leaf of a row holds four
    poses, the middle two at the same distance from the centre -- a planted exact tie in every full leaf.  ids are NOT positions (3 p + 7).
    -> (poses (n, 6) float32, ids (n,) int32)"""
    rng = np.random.default_rng(seed)
    p = np.arange(n)
    row, col = p // 100, p % 100
    col = np.where(row % 2 == 0, col, 99 - col)
    poses = np.zeros((n, 6), F)
    poses[:, 0] = F(1 / 16) + col.astype(F) / F(8)
    poses[:, 1] = F(1 / 16) + row.astype(F) / F(8)
    poses[:, 2] = rng.integers(0, 3, n).astype(F) / F(16)
    poses[:, 5] = np.where(row % 2 == 0, 0.0, np.pi).astype(F)
    return poses, (3 * p + 7).astype(np.int32)


STORE_SIZES = (1, 2, 65, 5000)


def square_drive(n=248, side_steps=60, step=0.5):
    """a square of side_steps * step metres driven counter-clockwise from the origin, one key pose per step; the drive RE-ENTERS its first side after one
    lap (n > 4 side_steps): the last poses lie where the first ones do.  ids = positions.  -> (poses, ids)"""
    p = np.arange(n) % (4 * side_steps)
    side, k = p // side_steps, (p % side_steps).astype(np.float64) * step
    s = side_steps * step
    x = np.select([side == 0, side == 1, side == 2, side == 3], [k, s, s - k, 0.0])
    y = np.select([side == 0, side == 1, side == 2, side == 3], [0.0, k, s, s - k])
    poses = np.zeros((n, 6), F)
    poses[:, 0], poses[:, 1] = x, y
    poses[:, 5] = (np.arange(n) // side_steps % 4 * (np.pi / 2)).astype(F)
    poses[:, 5] = np.where(poses[:, 5] > np.pi, poses[:, 5] - F(2 * np.pi), poses[:, 5])
    return poses, np.arange(n, dtype=np.int32)


SQUARE_MINIMA = dict(n_in_radius=30, qualify=8, nearer_skipped_for_id=1)


def tiny_cloud(key, n=4):
    """n body-frame points {x, y, z, c} of keyframe `key` (what the selection tests push: the clouds' content is not their subject)"""
    rng = np.random.default_rng(1000 + int(key))
    return rng.uniform(-1, 1, (n, 4)).astype(F)
