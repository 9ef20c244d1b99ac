"""Inputs of the nearest-neighbour and association tests (test_nn_reference.py / test_assoc_reference.py without a GPU,
test_gpu_nearest.py / test_gpu_association.py with one): built once here so that the case the oracle was checked on is the case the
kernel sees.  Lattice clouds are integer coordinates in units of nn_reference.STEP (64 units per metre)."""
from __future__ import annotations

import numpy as np

import nn_reference as nnr

U = 64                                   # lattice units per metre
RES = (0.3, 0.5, 0.7, 1.0, 1.9, 3.0)     # target-grid cell sizes of the score tests (0.3, 0.7, 1.9 and 3.0 are not powers of two)


def _uniq(I, rng):
    I = np.unique(np.asarray(I, np.int64), axis=0)
    return I[rng.permutation(len(I))]


def slab(seed, n, box=(20, 20, 2), centre=(0, 0, 0)):
    """about n distinct random lattice points in a box (metres)"""
    rng = np.random.default_rng(seed)
    I = np.stack([rng.integers(-b * U // 2, b * U // 2 + 1, n) + c * U for b, c in zip(box, centre)], axis=1)
    return _uniq(I, rng)


def exactly(I, n, seed):
    """exactly n distinct lattice points: I topped up / cut"""
    rng = np.random.default_rng(seed)
    I = _uniq(I, rng)
    while len(I) < n:
        extra = I[rng.integers(0, len(I), n - len(I))] + rng.integers(-3, 4, (n - len(I), 3))
        I = _uniq(np.concatenate([I, extra]), rng)
    return I[:n]


def pose(R=None, t=(0, 0, 0)):
    """an integer rotation (signed permutation, det +1) and a lattice translation -> (R int, t int, T float32 4x4)"""
    R = np.eye(3, dtype=np.int64) if R is None else np.asarray(R, np.int64)
    assert round(np.linalg.det(R)) == 1 and (np.abs(R).sum(0) == 1).all()
    t = np.asarray(t, np.int64)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R, t * nnr.STEP
    return R, t, T


RZ90 = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
RX180 = [[1, 0, 0], [0, -1, 0], [0, 0, -1]]


def moved(Iq, R, t):
    return np.asarray(Iq, np.int64) @ np.asarray(R, np.int64).T + np.asarray(t, np.int64)


# ---- score: lattice cases ------------------------------------------------------------------------------------------------------------
def fitness_lattice_cases():
    """list of dict(name, It, Iq, R, t, T, census_res, need): the census (at every cell size in census_res, of the MOVED source) must
    hold at least need[class] queries"""
    out = []

    def add(name, It, Iq, R=None, t=(0, 0, 0), census_res=(1.0,), need=None):
        R, t, T = pose(R, t)
        out.append(dict(name=name, It=It, Iq=Iq, R=R, t=t, T=T, census_res=census_res, need=need or {}))

    rng = np.random.default_rng(11)
    dense = slab(1, 45000)                                 # more than 32 768 points: the grid route, cube growth and all
    near = dense[rng.integers(0, len(dense), 8000)] + rng.integers(-4, 5, (8000, 3))
    add("dense_slab", dense, near, census_res=(1.0, 1.9, 3.0), need=dict(own_cell=5000))
    add("dense_slab_rz90_shift", dense, near, R=RZ90, t=(32, -64, 16), census_res=(1.0,), need=dict(own_cell=2000, block=5000, far=100))
    add("dense_slab_rx180", dense, near, R=RX180, t=(0, 16, -8), census_res=(1.0,), need=dict(own_cell=2000, block=5000))
    # a thin sheet and poles: the nearest of a point above the sheet lies across its cell's walls
    g = np.arange(-12 * U, 12 * U + 1, 16)
    sheet = np.stack(np.meshgrid(g, g, [0], indexing="ij"), -1).reshape(-1, 3)
    px = rng.integers(-11 * U, 11 * U, (40, 2))
    poles = np.concatenate([np.stack([np.full(48, x), np.full(48, y), np.arange(4, 4 * 49, 4)], 1) for x, y in px])
    sp = _uniq(np.concatenate([sheet, poles]), rng)
    above = np.stack([rng.integers(-12 * U, 12 * U, 6000), rng.integers(-12 * U, 12 * U, 6000), rng.integers(12, 100, 6000)], 1)
    add("sheet_and_poles", sp, above, census_res=(1.0,), need=dict(block=1500, far=3000))
    # a map with a side cut away and a source several cells off what is left; two anchors keep the cut-away side inside the grid
    cut = dense[dense[:, 0] < 0]
    cut = np.concatenate([cut, [[10 * U, 10 * U, U], [10 * U, -10 * U, -U]]])
    off = np.stack([rng.integers(2 * U, 8 * U, 2000), rng.integers(-8 * U, 8 * U, 2000), rng.integers(-U, U, 2000)], 1)
    add("cut_map_far_source", cut, off, census_res=(0.3, 0.5, 1.0), need=dict(far=1900))
    big = slab(2, 90000)
    big = np.concatenate([big[big[:, 0] < 0], [[10 * U, 10 * U, U], [10 * U, -10 * U, -U]]])
    add("cut_big_map_far_source", big, off[:1000], census_res=(0.3, 0.5, 1.0), need=dict(far=950))
    add("source_above_map", dense, near[:2000], t=(0, 0, 5 * U), census_res=(0.3, 0.5), need=dict(outside=2000))
    # a source wholly outside the target's box on one, two, three axes
    core = near[(np.abs(near[:, :2]) < 3 * U).all(axis=1)][:600]
    for k, sh in enumerate([(20 * U, 0, 0), (20 * U, -20 * U, 0), (-20 * U, 20 * U, 12 * U)], 1):
        add(f"outside_{k}_axes", dense, core, t=sh, census_res=(0.3, 1.0, 3.0), need=dict(outside=600))
    # target points ON cell walls (c + 0.5) * res of the 0.5 m and 1.0 m grids, queries straight across the wall
    w = np.concatenate([16 + 32 * np.arange(-16, 16), 32 + 64 * np.arange(-8, 8)])
    wt = _uniq(np.stack([rng.choice(w, 4000), rng.choice(w, 4000), rng.choice(w, 4000)], 1), rng)
    base = wt[rng.integers(0, len(wt), 6000)]
    axis, step = rng.integers(0, 3, 6000), rng.choice([-40, -17, -5, -2, -1, 1, 2, 5, 17, 40], 6000)
    across = base.copy()
    across[np.arange(6000), axis] += step
    add("points_on_walls", wt, across, census_res=(0.5, 1.0), need=dict(block=3000, own_cell=100, far=500))
    # cell populations that walk the candidate loop's tails: cells of the 1 m grid holding exactly 1, 7, 8, 9, 15, 16, 17 points
    pts, qs = [], []
    pops = (1, 7, 8, 9, 15, 16, 17)
    for j, c in enumerate(np.stack(np.meshgrid(np.arange(-6, 6), np.arange(-6, 6), [0, 1], indexing="ij"), -1).reshape(-1, 3)):
        lo = 32 + 64 * c                                   # the cell is [lo, lo + 64) per axis
        inside = _uniq(rng.integers(1, 63, (64, 3)), rng)[:pops[j % len(pops)]]
        pts.append(lo + inside)
        qs.append(lo + rng.integers(0, 64, (12, 3)))
    add("cell_population_tails", np.concatenate(pts), np.concatenate(qs), census_res=(1.0,), need=dict(own_cell=500, block=500))
    return out


TAIL_POPULATIONS = (1, 7, 8, 9, 15, 16, 17)


def wall_ulp_case(res, seed=5):
    """(target, source) float32, NOT on the lattice along x: target x within one fp32 ulp on either side of a wall (c + 0.5) * res (and on
    the fp32 nearest to it), y and z on the lattice; queries at the same y, z straight across the wall.  Keys are dx^2 alone."""
    rng = np.random.default_rng(seed)
    n = 3000
    c = rng.integers(-20, 20, n)
    wall = ((c + 0.5) * res).astype(np.float32)
    x = np.where(rng.integers(0, 3, n) == 0, wall, np.where(rng.integers(0, 2, n) == 0, np.nextafter(wall, np.float32(-np.inf)),
                                                            np.nextafter(wall, np.float32(np.inf)))).astype(np.float32)
    yz = rng.integers(-6 * U, 6 * U, (n, 2)) * 8            # 0.125 m apart at least: a point's nearest is its own partner
    t = np.concatenate([x[:, None], nnr.lattice(yz)], axis=1).astype(np.float32)
    t = t[np.unique(yz, axis=0, return_index=True)[1]]
    s = t.copy()
    s[:, 0] += (rng.choice([-1, 1], len(s)) * rng.choice([2.0 ** -12, 2.0 ** -9, 0.01, 0.03], len(s))).astype(np.float32)
    return t, s


# ---- score: the small-map route -----------------------------------------------------------------------------------------------------
SMALL_NT = (32767, 32768, 32769, 511, 512, 513, 575, 576, 577)
FAR_FRACTIONS = (0.0, 0.02, 0.5, 1.0)


def small_map_case(nt, far_frac, ns, seed=0):
    """(It, Iq): a target of exactly nt points -- a slab on x < 0 and two anchors that keep x > 0 inside the grid -- and ns queries of which
    far_frac lie in the empty half (own cell empty: `far`), the rest within a few units of a target point"""
    rng = np.random.default_rng(1000 + seed + nt)
    half = slab(seed + nt, int(nt * 1.2) + 16, box=(6, 12, 2), centre=(-4, 0, 0))
    It = exactly(half, nt - 2, seed)
    It = np.concatenate([It, [[8 * U, 7 * U, U], [8 * U, -7 * U, -U]]])
    It = It[rng.permutation(nt)]
    n_far = int(round(far_frac * ns))
    pick = It[rng.integers(0, nt, ns - n_far)]
    nearq = pick + rng.integers(-2, 3, (ns - n_far, 3))
    # a jitter that carries a query into an empty cell of the 1 m grid would make it `far`: such a query stays on its target point
    occupied = set(map(tuple, nnr.cells(nnr.lattice(It), 1.0).tolist()))
    stay = np.fromiter((tuple(c) not in occupied for c in nnr.cells(nnr.lattice(nearq), 1.0).tolist()), bool, len(nearq))
    nearq[stay] = pick[stay]
    farq = np.stack([rng.integers(2 * U, 6 * U, n_far), rng.integers(-5 * U, 5 * U, n_far), rng.integers(-U // 2, U // 2, n_far)], 1)
    Iq = np.concatenate([nearq, farq])
    return It, Iq[rng.permutation(ns)]


# ---- ICP ------------------------------------------------------------------------------------------------------------------------------
def icp_gate_case(gate, seed=3):
    """isolated target points on a coarse grid; per point queries at an axis offset of floor(gate / STEP) units (kept: ON the gate when the
    gate is a lattice distance) and one unit beyond (dropped), and queries well inside.  -> (Is, It)"""
    rng = np.random.default_rng(seed)
    k = int(np.floor(gate / nnr.STEP))
    s = max(4 * (k + 1), 2 * U)
    half = max(1, min(4, (24 * U) // s))
    g = np.arange(-half, half + 1) * s
    It = _uniq(np.stack(np.meshgrid(g, g, g[: max(2, len(g) // 2)], indexing="ij"), -1).reshape(-1, 3), rng)
    qs = []
    for p in It:
        for a in range(3):
            for sg in (-1, 1):
                for off in (k, k + 1):
                    q = p.copy()
                    q[a] += sg * off
                    qs.append(q)
        r = max(2, k // 3)
        qs.extend(p + rng.integers(-r, r + 1, (6, 3)))
    Is = np.asarray(qs, np.int64)
    return Is[rng.permutation(len(Is))], It


ICP_GATES = (0.25, 0.5, 2.0, 10.0, 0.3)


def icp_tie_case(seed=4):
    """a coarse lattice (every 16th unit) in a permuted order; sources half a step off on one, two or three axes: two, four, eight exactly
    equidistant nearest points.  -> (Is, It)"""
    rng = np.random.default_rng(seed)
    g = np.arange(-12, 13) * 16
    It = _uniq(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3), rng)
    n = 2400
    base = It[rng.integers(0, len(It), n)]
    off = np.zeros((n, 3), np.int64)
    kind = rng.integers(0, 4, n)                           # 0: a small offset (no tie); 1..3: half a step on that many axes
    for i in range(n):
        if kind[i] == 0:
            off[i] = rng.integers(-5, 6, 3)
        else:
            ax = rng.permutation(3)[:kind[i]]
            off[i, ax] = 8
            rest = np.setdiff1d(np.arange(3), ax)
            off[i, rest] = rng.integers(-3, 4, len(rest))
    Is = base + off
    inside = (np.abs(Is) <= 12 * 16).all(axis=1)
    return Is[inside], It


def icp_few_case(n_kept, seed=6):
    """a source of which all but n_kept points lie beyond a 0.5 m gate -> (Is, It, gate)"""
    rng = np.random.default_rng(seed)
    It = slab(seed, 3000, box=(10, 10, 2))
    close = It[rng.integers(0, len(It), n_kept)] + np.array([[3, 0, 0], [0, -2, 1], [1, 1, -2], [0, 0, 0]])[:n_kept] if n_kept else np.zeros((0, 3), np.int64)
    away = np.stack([rng.integers(-5 * U, 5 * U, 500), rng.integers(-5 * U, 5 * U, 500), rng.integers(3 * U, 9 * U, 500)], 1)
    Is = np.concatenate([close, away]).astype(np.int64)
    return Is[rng.permutation(len(Is))], It, 0.5


def icp_degenerate_case(shape, seed=8):
    """kept correspondences that are all in one plane (z = 0) or on one line (y = z = 0); everything else is beyond the 0.5 m gate"""
    rng = np.random.default_rng(seed)
    if shape == "planar":
        g = np.arange(-20, 21) * 32
        It = np.stack(np.meshgrid(g, g, [0], indexing="ij"), -1).reshape(-1, 3)
        Is = It[rng.integers(0, len(It), 600)] + np.concatenate([rng.integers(-6, 7, (600, 2)), np.zeros((600, 1), np.int64)], 1)
    else:
        It = np.stack([np.arange(-300, 301) * 8, np.zeros(601, np.int64), np.zeros(601, np.int64)], 1)
        Is = It[rng.integers(0, len(It), 400)] + np.concatenate([rng.integers(-3, 4, (400, 1)), np.zeros((400, 2), np.int64)], 1)
    away = np.stack([rng.integers(-5 * U, 5 * U, 200), rng.integers(-5 * U, 5 * U, 200), rng.integers(6 * U, 9 * U, 200)], 1)
    It = _uniq(It, rng)
    return np.concatenate([Is, away]), It, 0.5


def icp_rank_one_case(shape, seed=14):
    """(src, tgt) float32 off the lattice whose first-iteration correlation has rank 1: a target of two points, or a target on one line
    (direction not along an axis) with the source on the same line"""
    rng = np.random.default_rng(seed)
    if shape == "two_points":
        tgt = np.array([[0.4071, -0.1733, 0.3119], [1.8137, -1.7009, -0.0941]], np.float32)
        src = (tgt[rng.integers(0, 2, 300)] + rng.normal(0, 0.05, (300, 3))).astype(np.float32)
        return src, tgt
    d = np.array([0.6, -0.64, 0.48])
    s = np.sort(rng.uniform(-9, 9, 500))
    tgt = (s[:, None] * d + [3.3, -1.7, 0.9]).astype(np.float64)
    src = tgt[rng.integers(0, 500, 300)] + rng.uniform(-0.2, 0.2, (300, 1)) * d
    return src.astype(np.float32), tgt.astype(np.float32)


def icp_loop_cases():
    """non-lattice (source, target, gate) from three generators: sheets and poles, a sparse field with a clump, a 2 000-point target"""
    out = []
    rng = np.random.default_rng(21)

    def drift(P, ang, t):
        c, s = np.cos(ang), np.sin(ang)
        R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ np.array([[1, 0, 0], [0, np.cos(ang / 3), -np.sin(ang / 3)], [0, np.sin(ang / 3), np.cos(ang / 3)]])
        return (P.astype(np.float64) @ R.T + np.asarray(t)).astype(np.float32)

    # sheets and poles: a floor, two walls, poles
    n = 9000
    floor = np.stack([rng.uniform(-15, 15, n), rng.uniform(-15, 15, n), rng.normal(0, 0.01, n)], 1)
    wall1 = np.stack([rng.uniform(-15, 15, n // 3), np.full(n // 3, 15.0) + rng.normal(0, 0.01, n // 3), rng.uniform(0, 4, n // 3)], 1)
    wall2 = np.stack([np.full(n // 3, -15.0) + rng.normal(0, 0.01, n // 3), rng.uniform(-15, 15, n // 3), rng.uniform(0, 4, n // 3)], 1)
    pol = np.concatenate([np.stack([np.full(60, x) + rng.normal(0, 0.01, 60), np.full(60, y) + rng.normal(0, 0.01, 60), rng.uniform(0, 5, 60)], 1)
                          for x, y in rng.uniform(-12, 12, (25, 2))])
    world = np.concatenate([floor, wall1, wall2, pol]).astype(np.float32)
    tgt = world[rng.permutation(len(world))[:12000]]
    src = drift(world[rng.permutation(len(world))[:3000]], 0.03, [0.25, -0.15, 0.05])
    out.append(dict(name="sheets_and_poles", src=src, tgt=tgt, gate=2.0))
    # a sparse field with a clump
    field = rng.uniform(-25, 25, (4000, 3)) * [1, 1, 0.1]
    clump = rng.normal(0, 0.6, (3000, 3)) + [5, -3, 1]
    world = np.concatenate([field, clump]).astype(np.float32)
    src = drift(world[rng.permutation(len(world))[:2500]] + rng.normal(0, 0.02, (2500, 3)), -0.02, [-0.2, 0.3, 0.02])
    out.append(dict(name="sparse_field_with_clump", src=src, tgt=world, gate=5.0))
    # a 2 000-point target
    small = (rng.uniform(-8, 8, (2000, 3)) * [1, 1, 0.25]).astype(np.float32)
    small[:, 2] += (0.3 * np.sin(small[:, 0] * 0.7) + 0.2 * np.cos(small[:, 1] * 0.9)).astype(np.float32)
    src = drift(small[rng.permutation(2000)[:1200]] + rng.normal(0, 0.01, (1200, 3)), 0.025, [0.12, 0.1, -0.04])
    out.append(dict(name="target_of_2000", src=src, tgt=small, gate=10.0))
    return out


# ---- association -----------------------------------------------------------------------------------------------------------------------
IDENT_Q = np.array([0.0, 0.0, 0.0, 1.0])


def _feat(I, rng):
    f = np.zeros((len(I), 4), np.float32)
    f[:, :3] = nnr.lattice(I)
    f[:, 3] = rng.uniform(0.5, 2.0, len(I)).astype(np.float32)
    return f


def _map4(I):
    m = np.zeros((len(I), 4), np.float32)
    m[:, :3] = nnr.lattice(I)
    return m


def assoc_lattice_cases():
    """list of dict(name, kind, map (n,4), feat (n,4), q, t, need): lattice maps with the identity pose or a lattice translation"""
    out = []
    rng = np.random.default_rng(31)

    def add(name, kind, Im, If, t=(0, 0, 0), **need):
        out.append(dict(name=name, kind=kind, map=_map4(Im), feat=_feat(np.asarray(If, np.int64) - np.asarray(t, np.int64), rng), q=IDENT_Q,
                        t=np.asarray(t, np.float64) * nnr.STEP, need=need))

    # rows of a coarse lattice: a feature half-way between two rows has exact ties for the 5th place (edge maps: lines along x)
    gx = np.arange(-40, 41) * 8
    rows_ = np.stack(np.meshgrid(gx, np.arange(-6, 7) * 48, np.arange(0, 3) * 48, indexing="ij"), -1).reshape(-1, 3)
    rows_ = _uniq(rows_, rng)
    f = rows_[rng.integers(0, len(rows_), 1500)] + np.stack([rng.choice([0, 4], 1500), rng.choice([0, 24, 5, -7], 1500), rng.choice([0, 24, 3], 1500)], 1)
    add("edge_rows_with_ties", "edge", rows_, f, ties=100, valid=300)
    add("edge_rows_shifted_pose", "edge", rows_, f, t=(64, -128, 32), ties=100, valid=300)
    # sheets of a coarse lattice (plane maps)
    gs = np.arange(-30, 31) * 16
    sheets = np.stack(np.meshgrid(gs, gs, [32, 192], indexing="ij"), -1).reshape(-1, 3)
    sheets = _uniq(sheets, rng)
    f = sheets[rng.integers(0, len(sheets), 1500)] + np.stack([rng.choice([0, 8, 3], 1500), rng.choice([0, 8, -5], 1500), rng.integers(-20, 21, 1500)], 1)
    add("plane_sheets_with_ties", "plane", sheets, f, ties=100, valid=300)
    # the 5th neighbour exactly ON the gate (invalid: the gate is strict) and one unit inside (valid by the gate)
    for kind, r2 in (("edge", 64 * 64), ("plane", 2 * 64 * 64)):
        Im, If, n_on = [], [], 0
        cen = np.stack(np.meshgrid(np.arange(-3, 4) * 6 * U, np.arange(-3, 4) * 6 * U, [96], indexing="ij"), -1).reshape(-1, 3)
        for j, c in enumerate(cen):
            # four near points and a fifth at squared distance exactly r2 (edge: 64 units along an axis; plane: 64 and 64 on two axes)
            if kind == "edge":
                four = c + np.array([[3, 0, 0], [-5, 1, 0], [9, 0, 1], [-12, -1, 0]])
                fifth = c + np.array([64, 0, 0])
            else:
                four = c + np.array([[10, 3, 2], [-14, 5, -1], [4, -20, 1], [-9, -11, 0]])
                fifth = c + np.array([64, 64, 0])
            Im.extend(four)
            Im.append(fifth)
            If.append(c)                                   # 5th exactly on the gate
            If.append(c + np.array([1, 0, 0]))             # one unit towards it: inside
            n_on += 1
        add(f"{kind}_fifth_on_gate", kind, np.asarray(Im), np.asarray(If), on_gate=n_on, gate_pass=n_on)
    # features outside the map's box on each axis and side, by less and by more than a cell
    box = slab(32, 6000, box=(8, 8, 3))
    f = []
    for a in range(3):
        for sg in (-1, 1):
            for by in (20, 50, 100, 200):                  # 0.3 .. 3.1 m beyond the face
                p = box[rng.integers(0, len(box), 40)].copy()
                p[:, a] = sg * ((8, 8, 3)[a] * U // 2 + by)
                f.append(p)
    f = np.concatenate(f)
    add("edge_features_outside_box", "edge", box, f, gate_pass=50)
    add("plane_features_outside_box", "plane", box, f, gate_pass=50)
    # maps of exactly 5, 6 and 64 points; a map whose points all share one cell
    for n in (5, 6, 64):
        tiny = exactly(slab(40 + n, n + 8, box=(1, 1, 1)), n, n)
        f = rng.integers(-80, 81, (200, 3))
        add(f"edge_map_of_{n}", "edge", tiny, f, gate_pass=1)
        add(f"plane_map_of_{n}", "plane", tiny, f, gate_pass=1)
    one = exactly(rng.integers(33, 95, (300, 3)), 200, 7)   # all inside the 1 m cell [0.5, 1.5)^3 and the sqrt(2) m cell [0.707, 2.12)^3
    one = one[(one > 46).all(axis=1)]
    f = rng.integers(0, 160, (300, 3))
    add("edge_map_in_one_cell", "edge", one, f, gate_pass=50)
    add("plane_map_in_one_cell", "plane", one, f, gate_pass=50)
    return out
