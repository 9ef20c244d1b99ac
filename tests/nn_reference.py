"""An independent reference for the exact 1-NN searches: the fitness score, the loop-closure ICP, and the k nearest of arbitrary queries
(numpy and scipy only; nothing from oracle/).

The product ranks candidates by the fp32 key ``((dx*dx + dy*dy) + dz*dz)`` and breaks ties by the smaller original index.
Candidates come from an fp64 ``cKDTree``; their keys are recomputed with float32 ufuncs (``knn_reference.fp32_keys``), ordered by
``(key, index)``, and a row is accepted only when it is PROVEN complete by the margin rule of ``knn_reference``; rows that fail the proof
fetch more candidates, nothing is guessed.

The lattice lever.  With target and source on the dyadic lattice ``STEP = 2^-6`` m and a pose that is the identity, a lattice translation
or a rotation by a multiple of 90 degrees about an axis, every fp32 operation of the transform and of the key is exact while the nearest
squared distance stays below 2^24 lattice units, the fp64 sum of up to 2^17 such keys is exact in any order, and the score is
``integer_sum * STEP^2 / n``: one division.  ``lattice_score`` computes that from integer coordinates in int64; a kernel's score on such
inputs must equal it bit for bit, and one query with a wrong neighbour changes it.
"""
from __future__ import annotations

import math

import numpy as np
from scipy.spatial import cKDTree

from knn_reference import fp32_keys

STEP = 2.0 ** -6
ICP_STATES = ("not_converged", "iterations", "transform", "abs_mse", "rel_mse", "no_correspondences")


def lattice(I) -> np.ndarray:
    """integer lattice coordinates -> float32 metres (exact: |I| < 2^24)"""
    I = np.asarray(I, np.int64)
    assert np.abs(I).max(initial=0) < 2 ** 24
    return (I.astype(np.float64) * STEP).astype(np.float32)


def nearest_k(target, queries, k: int, extra: int = 8):
    """(idx (nq, k) int64, key (nq, k) float32): the k nearest target points of every query, each row ordered by (key, index)"""
    T = np.ascontiguousarray(np.asarray(target, np.float32)[:, :3])
    Q = np.ascontiguousarray(np.asarray(queries, np.float32)[:, :3])
    nt, nq = T.shape[0], Q.shape[0]
    if not 1 <= k <= nt:
        raise ValueError(f"need 1 <= k <= n_target (k={k}, n_target={nt})")
    both = np.concatenate([T, Q])                         # fp32_keys indexes one array: queries are rows nt.. of it
    T64, Q64 = T.astype(np.float64), Q.astype(np.float64)
    tree = cKDTree(T64)
    margin = 16.0 * float(np.spacing(np.float32(max(float(np.abs(both).max()), 1.0))))
    idx_out = np.empty((nq, k), np.int64)
    key_out = np.empty((nq, k), np.float32)
    rows = np.arange(nq)
    m = min(nt, k + extra)
    while rows.size:
        d64, cand = tree.query(Q64[rows], k=m)
        d64, cand = d64.reshape(rows.size, m), cand.reshape(rows.size, m)
        key = fp32_keys(both, nt + rows, cand)
        o = np.lexsort((cand, key), axis=-1)[:, :k]
        ki, kk = np.take_along_axis(cand, o, axis=1), np.take_along_axis(key, o, axis=1)
        if m == nt:
            done = np.ones(rows.size, bool)
        else:
            done = d64[:, -1] > np.sqrt(kk[:, -1].astype(np.float64)) + margin
        idx_out[rows[done]] = ki[done]
        key_out[rows[done]] = kk[done]
        rows = rows[~done]
        m = min(nt, 2 * m)
    return idx_out, key_out


def nearest(target, queries):
    """(index (nq,) int64, key (nq,) float32) of the nearest target point under (key, index)"""
    i, k = nearest_k(target, queries, 1)
    return i[:, 0], k[:, 0]


def lattice_nearest_d2(It, Iq) -> np.ndarray:
    """int64 (nq,): squared nearest distance in lattice units, from integer coordinates alone"""
    It, Iq = np.asarray(It, np.int64), np.asarray(Iq, np.int64)
    # integers below 2^24 and their squared distances below 2^53 are exact in fp64, sqrt is monotone: the tree's nearest IS a nearest
    _, j = cKDTree(It.astype(np.float64)).query(Iq.astype(np.float64), k=1)
    d = Iq - It[j]
    return (d * d).sum(axis=1)


def lattice_score(It, Iq) -> float:
    """mean squared 1-NN distance (m^2) of lattice queries Iq against lattice target It: exact integer sum, one division"""
    d2 = lattice_nearest_d2(It, Iq)
    n = len(d2)
    assert int(d2.max()) < 2 ** 24, f"nearest squared distance {int(d2.max())} units: fp32 keys are no longer exact"
    assert n <= 2 ** 17, f"{n} queries: the fp64 sum is no longer exact in any order"
    assert max(np.abs(It).max(), np.abs(Iq).max()) < 2 ** 12, "coordinates beyond 64 m: a product of a coordinate difference may round"
    return float(int(d2.sum())) * STEP ** 2 / n


def transform_f32(pts, T) -> np.ndarray:
    """((m0*x + m1*y) + m2*z) + m3 per row with float32 ufuncs, the product's association order"""
    T = np.asarray(T, np.float32).reshape(4, 4)
    P = np.asarray(pts, np.float32)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1).astype(np.float32)


def score(target, source, T=None) -> float:
    """getFitnessScore at any fp32 pose: fp32 transform, exact nearest, keys summed in fp64 (fsum: correctly rounded), / n"""
    src = np.asarray(source, np.float32)[:, :3]
    moved = src if T is None else transform_f32(src, T)
    _, key = nearest(target, moved)
    return math.fsum(key.astype(np.float64).tolist()) / len(key)


def kabsch(p, q):
    """R, t minimising sum |R p + t - q|^2, with the reflection fix: R = V diag(1, 1, det(V U^T)) U^T"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    cp, cq = p.mean(0), q.mean(0)
    U, s, Vt = np.linalg.svd((p - cp).T @ (q - cq))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, cq - R @ cp, s


def _T32(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R.astype(np.float32), t.astype(np.float32)
    return T


def icp_first_iteration(source, target, gate: float) -> dict:
    """One iteration from the identity guess.  A query is kept when key <= gate^2, with gate^2 the fp64 product gate * gate and the fp32
    key widened to fp64 (k_icp_accumulate's `(double)best <= max_d2`, max_d2 = max_dist * max_dist).  Fewer than 3 kept: state 5, T = I."""
    src = np.asarray(source, np.float32)[:, :3]
    tgt = np.asarray(target, np.float32)[:, :3]
    idx, key = nearest(tgt, src)
    gate2 = float(gate) * float(gate)
    keep = key.astype(np.float64) <= gate2
    n = int(keep.sum())
    p, q = src[keep].astype(np.float64), tgt[idx[keep]].astype(np.float64)
    out = dict(idx=idx, key=key, keep=keep, n=n, sum_p=p.sum(0), sum_q=q.sum(0), sum_pq=p.T @ q,
               sum_d2=math.fsum(key[keep].astype(np.float64).tolist()), gate2=gate2)
    if n < 3:
        out.update(T=np.eye(4, dtype=np.float32), state=5, iterations=0, singular=None)
        return out
    R, t, s = kabsch(p, q)
    out.update(T=_T32(R, t), state=1, iterations=1, singular=s)
    return out


def _compose_f32(T, fin):
    """fin <- T * fin with a float32 accumulator, k ascending"""
    nf = np.zeros((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            v = np.float32(0.0)
            for k in range(4):
                v = np.float32(v + np.float32(T[i, k] * fin[k, j]))
            nf[i, j] = v
    return nf


def icp_align(source, target, gate=10.0, max_iterations=100, transformation_eps=1e-6, fitness_eps=1e-6):
    """pcl::IterativeClosestPoint with DefaultConvergenceCriteria as include/rgc_hip.h documents it: per iteration the exact nearest of
    every (already transformed, fp32) source point, kept when key <= gate^2; fewer than 3 -> NO_CORRESPONDENCES; Kabsch; the source and
    the running transform updated in fp32; then in this order: the iteration cap, the transform test (cos(angle) >= 1 - eps and |t|^2 <=
    eps on the fp32 increment), |mse - previous| < 1e-12, the relative change of the correspondence MSE < eps.
    Returns (final_T float32 4x4, dict(iterations, state, converged, n_correspondences, fitness))."""
    src = np.asarray(source, np.float32)[:, :3]
    tgt = np.asarray(target, np.float32)[:, :3]
    cur = src.copy()
    fin = np.eye(4, dtype=np.float32)
    gate2 = float(gate) * float(gate)
    prev, it, state, n = np.finfo(np.float64).max, 0, 0, 0
    while True:
        idx, key = nearest(tgt, cur)
        key64 = key.astype(np.float64)
        keep = key64 <= gate2
        n = int(keep.sum())
        if n < 3:
            state = 5
            break
        R, t, _ = kabsch(cur[keep], tgt[idx[keep]])
        T = _T32(R, t)
        cur = transform_f32(cur, T)
        fin = _compose_f32(T, fin)
        it += 1
        if it >= max_iterations:
            state = 1
            break
        cos_angle = 0.5 * (float(T[0, 0]) + float(T[1, 1]) + float(T[2, 2]) - 1.0)
        tr2 = float(T[0, 3]) ** 2 + float(T[1, 3]) ** 2 + float(T[2, 3]) ** 2
        if cos_angle >= 1.0 - transformation_eps and tr2 <= transformation_eps:
            state = 2
            break
        mse = math.fsum(key64[keep].tolist()) / n
        if abs(mse - prev) < 1e-12:
            state = 3
            break
        if abs(mse - prev) / prev < fitness_eps:
            state = 4
            break
        prev = mse
    return fin, dict(iterations=it, state=state, converged=int(state != 5), n_correspondences=n, fitness=score(tgt, src, fin))


def cells(xyz, res: float) -> np.ndarray:
    """the documented cell rule, floor(x / res - 0.5) per axis, in fp64 from the fp32 coordinates"""
    return np.floor(np.asarray(xyz, np.float32)[:, :3].astype(np.float64) / float(res) - 0.5).astype(np.int64)


def query_class(target, queries, res: float, gate=None) -> dict:
    """A geometric census from the cell rule alone; boolean masks per query.  Exactly one of
      outside   more than one cell outside the target's box of cells on some axis
      far       (else) own cell holds no target point, or the nearest is not nearer than the surface of the 3x3x3 block of cells
      own_cell  (else) the nearest is nearer than the nearest wall of the own cell
      block     (else)
    and with a gate: beyond_gate (key > gate^2), on_gate (key == gate^2 exactly).  It says what a case contains, not which instruction
    path a kernel took."""
    T = np.asarray(target, np.float32)[:, :3]
    Q = np.asarray(queries, np.float32)[:, :3]
    res = float(res)
    ct, cq = cells(T, res), cells(Q, res)
    lo, hi = ct.min(0), ct.max(0)
    outside = ((cq < lo - 1) | (cq > hi + 1)).any(axis=1)
    occupied = set(map(tuple, ct.tolist()))
    own_has = np.fromiter((tuple(c) in occupied for c in cq.tolist()), bool, len(cq))
    _, key = nearest(T, Q)
    d = np.sqrt(key.astype(np.float64))
    q64 = Q.astype(np.float64)
    wall_lo = (cq + 0.5) * res
    own_wall = np.minimum(q64 - wall_lo, wall_lo + res - q64).min(axis=1)
    block_wall = np.minimum(q64 - (wall_lo - res), wall_lo + 2 * res - q64).min(axis=1)
    far = ~outside & (~own_has | (d >= block_wall))
    own = ~outside & ~far & (d < own_wall)
    out = dict(outside=outside, far=far, own_cell=own, block=~outside & ~far & ~own, key=key)
    if gate is not None:
        g2 = float(gate) * float(gate)
        k64 = key.astype(np.float64)
        out.update(beyond_gate=k64 > g2, on_gate=k64 == g2)
    return out


def census(target, queries, res: float, gate=None) -> dict:
    """counts per class of query_class"""
    return {k: int(v.sum()) for k, v in query_class(target, queries, res, gate).items() if k != "key"}


def cell_histogram(target, res: float) -> np.ndarray:
    """points per occupied cell"""
    _, cnt = np.unique(cells(target, res), axis=0, return_counts=True)
    return cnt


def t_tolerance(T) -> float:
    """4 fp32 ulps of the largest entry of T: one fp32 rounding of a product of fp64 factors, plus slack"""
    return 4.0 * float(np.spacing(np.float32(np.abs(np.asarray(T, np.float32)).max())))


def sum_reorder_bound(n: int) -> float:
    """relative bound on re-ordering a sum of n non-negative fp64 terms"""
    return n * 2.0 ** -52


def rigid_residual(T, p, q) -> float:
    """sum |R p + t - q|^2 in fp64 for a 4x4 T"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    e = np.asarray(p, np.float64) @ T[:3, :3].T + T[:3, 3] - np.asarray(q, np.float64)
    return float((e * e).sum())


def check_rigid(T, ref: dict, source, target) -> None:
    """What holds for the first iteration's T even where Kabsch is not unique (a rank-1 correlation: a target of two points, a kept set on
    one line): a proper rotation, and the optimum's residual.  An fp32 T moves a residual e by |dT| |p| <= 2^-23 * (|p| + 1) per
    point, the sum of squares by 2 |e| |de| per point: a relative 1e-4 covers clouds within 64 m whose residual is above a millimetre;
    the absolute term covers exact fits."""
    R = np.asarray(T, np.float64)[:3, :3]
    assert abs(np.linalg.det(R) - 1) < 1e-5 and np.abs(R @ R.T - np.eye(3)).max() < 1e-5, f"not a proper rotation: det {np.linalg.det(R)!r}"
    keep = ref["keep"]
    p, q = np.asarray(source, np.float32)[keep, :3], np.asarray(target, np.float32)[ref["idx"][keep], :3]
    got, best = rigid_residual(T, p, q), rigid_residual(ref["T"], p, q)
    assert got <= best * (1 + 1e-4) + 1e-9 * len(p), f"residual {got!r}, the optimum's {best!r}"
