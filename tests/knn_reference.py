"""An independent reference for exact k-NN and neighbourhood covariances (numpy and scipy only; nothing from oracle/).

The product ranks a query's neighbours by the fp32 key ``((dx*dx + dy*dy) + dz*dz)`` -- flann::L2_Simple<float>, no FMA -- and breaks
ties by ascending index.  Here candidates come from an fp64 ``scipy.spatial.cKDTree``; their fp32 keys are recomputed with
numpy float32 arrays (separate multiply and add ufuncs: nothing is contracted) and ordered by ``(key, index)``.  A row is accepted only
when it is PROVEN complete: the fp64 distance of the last candidate fetched exceeds ``sqrt(k-th key)`` by a margin of a few fp32 ulps of
the largest coordinate, so every point not fetched has a larger key than the k-th.  Rows that fail the proof fetch more candidates
(up to the whole cloud); nothing is guessed.  The query is a candidate of its own row like any other point: with more than k exact
copies of it, the tie rule may leave it out.

Covariances follow fast_gicp_impl.hpp:256-293 in fp64: the mean-centred sum over the k neighbours divided by k, then NONE (that matrix),
PLANE (``U diag(1, 1, 1e-3) U^T`` from ``np.linalg.eigh``) and MIN_EIG (eigenvalues clamped below at 1e-3).  PLANE depends on the normal,
which is defined only where the two smallest eigenvalues differ: ``eigengap`` gives ``(l2 - l3) / trace`` per row to decide where it is.
"""
from __future__ import annotations

import numpy as np
from scipy.spatial import cKDTree

GAP_MIN = 1e-6      # PLANE is compared only where (l2 - l3) / trace is at least this


def fp32_keys(P: np.ndarray, q: np.ndarray, cand: np.ndarray) -> np.ndarray:
    """((dx*dx + dy*dy) + dz*dz) in float32 for query rows q (m,) against candidates cand (m, c)"""
    P = np.asarray(P, np.float32)
    d = P[q][:, None, :] - P[cand]                       # float32 - float32: rounded once
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return (dx * dx + dy * dy) + dz * dz                 # float32 ufuncs, evaluated in this order


def knn(xyz, k: int, extra: int = 8):
    """Exact k nearest neighbours of every point of xyz (n, >=3) among the same points under the product's rule.
    Returns (idx (n, k) int64, key (n, k) float32), each row ordered by (key, index)."""
    P = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
    n = P.shape[0]
    if not 1 <= k <= n:
        raise ValueError(f"need 1 <= k <= n (k={k}, n={n})")
    P64 = P.astype(np.float64)
    tree = cKDTree(P64)
    # an fp32 key differs from the exact squared distance by a few relative ulps; in distance that is a few ulps of the largest coordinate
    margin = 16.0 * float(np.spacing(np.float32(max(float(np.abs(P).max()), 1.0))))
    idx_out = np.empty((n, k), np.int64)
    key_out = np.empty((n, k), np.float32)
    rows = np.arange(n)
    m = min(n, k + extra)
    while rows.size:
        d64, cand = tree.query(P64[rows], k=m)
        d64, cand = d64.reshape(rows.size, m), cand.reshape(rows.size, m)
        key = fp32_keys(P, rows, cand)
        o = np.lexsort((cand, key), axis=-1)[:, :k]
        ki, kk = np.take_along_axis(cand, o, axis=1), np.take_along_axis(key, o, axis=1)
        if m == n:
            done = np.ones(rows.size, bool)
        else:
            done = d64[:, -1] > np.sqrt(kk[:, -1].astype(np.float64)) + margin
        idx_out[rows[done]] = ki[done]
        key_out[rows[done]] = kk[done]
        rows = rows[~done]
        m = min(n, 2 * m)
    return idx_out, key_out


def sample_covariances(xyz, idx) -> np.ndarray:
    """fp64 (n, 3, 3): sum over the neighbours of (p - mean)(p - mean)^T, divided by k (fast_gicp_impl.hpp:256-262)"""
    P = np.asarray(xyz, np.float32)[:, :3].astype(np.float64)
    N = P[np.asarray(idx)]                               # (n, k, 3)
    D = N - N.mean(axis=1, keepdims=True)
    return np.einsum("nki,nkj->nij", D, D) / N.shape[1]


def eigengap(S) -> np.ndarray:
    """(l2 - l3) / trace per row (l1 >= l2 >= l3); 0 where the trace is 0"""
    w = np.linalg.eigvalsh(S)                            # ascending
    tr = np.trace(S, axis1=1, axis2=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (w[:, 1] - w[:, 0]) / tr
    return np.where(tr > 0, g, 0.0)


def regularize(S, method: str) -> np.ndarray:
    """fast_gicp_impl.hpp:262-293 for method in ("NONE", "PLANE", "MIN_EIG")"""
    S = np.asarray(S, np.float64)
    if method == "NONE":
        return S.copy()
    w, U = np.linalg.eigh(S)                             # ascending: column 0 belongs to the smallest eigenvalue
    if method == "PLANE":
        vals = np.broadcast_to(np.array([1e-3, 1.0, 1.0]), w.shape)
    elif method == "MIN_EIG":
        vals = np.maximum(w, 1e-3)
    else:
        raise ValueError(method)
    return np.einsum("nij,nj,nkj->nik", U, vals, U)


def normals(S) -> np.ndarray:
    """unit eigenvector of the smallest eigenvalue (sign undefined)"""
    return np.linalg.eigh(np.asarray(S, np.float64))[1][:, :, 0]


def covariances(xyz, k: int, method: str = "PLANE"):
    """(cov (n, 3, 3), gap (n,), idx (n, k), key (n, k)): the whole chain on one cloud"""
    idx, key = knn(xyz, k)
    S = sample_covariances(xyz, idx)
    return regularize(S, method), eigengap(S), idx, key


def row_rel_err(a, b) -> np.ndarray:
    """per row: max |a - b| over the 3x3 divided by max |b| over the 3x3 (inf where b is 0 and a is not; 0 where both are 0)"""
    a, b = np.asarray(a, np.float64).reshape(len(a), -1), np.asarray(b, np.float64).reshape(len(b), -1)
    num, den = np.abs(a - b).max(axis=1), np.abs(b).max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = num / den
    return np.where(num == 0, 0.0, np.where(den > 0, r, np.inf))
