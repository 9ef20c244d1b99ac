"""An independent reference for the search index (rgc_search_knn / rgc_search_radius): numpy and scipy only, nothing from oracle/ and nothing from
the product.

It wraps the two references whose rows are PROVEN complete under the product's key -- nn_reference.nearest_k (the k nearest of arbitrary queries)
and gicp_mp_reference.radius_rows (every point with key < r2, strict): fp64 cKDTree supersets, fp32 keys recomputed with float32 ufuncs, the margin
rule, more candidates fetched until the proof holds -- and adds what the entry points define on top: the (key, index) order of a radius row, the
max_nn cut, the sentinel form of a row shorter than k (idx -1, key +inf behind min(k, n)), a brute-force all-pairs check that pins the wrappers
themselves on small cases, and a census of what a case contains."""
from __future__ import annotations

import numpy as np

import gicp_mp_reference as mr
import nn_reference as nn


def _xyz(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)[:, :3])


def knn_rows(target, queries, k: int):
    """(idx (nq, k) int32, key (nq, k) float32): the min(k, n) nearest under (key, index), then -1 / +inf"""
    T, Q = _xyz(target), _xyz(queries)
    m = min(int(k), len(T))
    idx = np.full((len(Q), k), -1, np.int32)
    key = np.full((len(Q), k), np.inf, np.float32)
    if len(Q) and m:
        i, d = nn.nearest_k(T, Q, m)
        idx[:, :m], key[:, :m] = i.astype(np.int32), d
    return idx, key


def radius_csr(target, queries, r: float, max_nn: int = 0):
    """(off (nq + 1,) int32, idx (m,) int32, key (m,) float32): rows ascending (key, index); max_nn > 0: the first max_nn of each row"""
    T, Q = _xyz(target), _xyz(queries)
    rows = mr.radius_rows(T, Q, r)
    row, idx, key = rows["row"], rows["idx"], rows["key"]
    o = np.lexsort((idx, key, row))
    row, idx, key = row[o], idx[o], key[o]
    start = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=len(Q)))])
    if max_nn > 0:
        keep = np.arange(len(row)) - start[row] < max_nn
        row, idx, key = row[keep], idx[keep], key[keep]
        start = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=len(Q)))])
    return start.astype(np.int32), idx.astype(np.int32), key.astype(np.float32)


def as_sets(off, idx, key):
    """a CSR result in the canonical (row, key, index) order: what an unsorted result is compared through"""
    row = np.repeat(np.arange(len(off) - 1), np.diff(off))
    o = np.lexsort((idx, key, row))
    return row[o], np.asarray(idx)[o], np.asarray(key)[o]


# ---- brute force: every pair's fp32 key, float32 ufuncs in the product's association ----
def all_keys(target, queries) -> np.ndarray:
    T, Q = _xyz(target), _xyz(queries)
    d = Q[:, None, :] - T[None, :, :]
    dd = d * d
    return ((dd[..., 0] + dd[..., 1]) + dd[..., 2]).astype(np.float32)


def brute_knn(target, queries, k: int):
    K = all_keys(target, queries)
    nq, n = K.shape
    ids = np.broadcast_to(np.arange(n), K.shape)
    o = np.lexsort((ids, K), axis=-1)[:, :k]
    idx = np.full((nq, k), -1, np.int32)
    key = np.full((nq, k), np.inf, np.float32)
    m = min(k, n)
    idx[:, :m], key[:, :m] = o[:, :m], np.take_along_axis(K, o[:, :m], axis=1)
    return idx, key


def brute_radius(target, queries, r: float, max_nn: int = 0):
    K = all_keys(target, queries)
    r2 = mr.r2_of(r)
    off, idx, key = [0], [], []
    for i in range(K.shape[0]):
        j = np.flatnonzero(K[i] < r2)
        j = j[np.lexsort((j, K[i, j]))]
        if max_nn > 0:
            j = j[:max_nn]
        idx.append(j)
        key.append(K[i, j])
        off.append(off[-1] + len(j))
    return np.asarray(off, np.int32), np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, np.int32), np.concatenate(key).astype(np.float32) if key else np.zeros(0, np.float32)


# ---- the census ----
def block_bound(target, queries, cell: float):
    """Per query: (bound, never).  bound = the distance to the nearest face of the 3 x 3 x 3 block of cells about the query's cell (clamped to one cell
    outside the grid) that is no border of the grid, inf if none; never = the block covers the grid.  The documented cell rule, floor(x / cell - 0.5)."""
    T, Q = _xyz(target), _xyz(queries)
    ct = nn.cells(T, cell)
    lo, dim = ct.min(0), ct.max(0) - ct.min(0) + 1
    c = np.clip(nn.cells(Q, cell) - lo, -1, dim)
    q = Q.astype(np.float64)
    bound = np.full(len(Q), np.inf)
    for a in range(3):
        low = q[:, a] - ((c[:, a] - 1 + lo[a]) + 0.5) * cell
        high = ((c[:, a] + 2 + lo[a]) + 0.5) * cell - q[:, a]
        bound = np.where(c[:, a] - 1 > 0, np.minimum(bound, low), bound)
        bound = np.where(c[:, a] + 1 < dim[a] - 1, np.minimum(bound, high), bound)
    never = np.maximum(c, dim - 1 - c).max(axis=1) <= 1
    return bound, never


def grow_census(target, queries, k: int, cell: float):
    """(must, cannot): queries whose k-th neighbour lies clearly beyond / clearly inside the 3 x 3 x 3 block at this cell size (a relative 1e-4 either
    side of the face: the kernel's own allowance is 1e-5), i.e. whose cube must / cannot grow.  A row that cannot fill (k > n) must grow unless the
    block covers the grid."""
    _, key = knn_rows(target, queries, k)
    bound, never = block_bound(target, queries, cell)
    kth = np.sqrt(key[:, -1].astype(np.float64))           # inf where the row is not full
    must = ~never & np.isfinite(bound) & (kth > bound * (1 + 1e-4))
    cannot = never | ~np.isfinite(bound) | (kth < bound * (1 - 1e-4))
    return int(must.sum()), int(cannot.sum())


def census(target, queries, ks=(), radii=(), window: int = 4096) -> dict:
    """what a case contains.  ks: k values; radii: (r, max_nn) pairs"""
    T, Q = _xyz(target), _xyz(queries)
    n = len(T)
    out = dict(outside=int(((Q < T.min(0)) | (Q > T.max(0))).any(axis=1).sum()), on_point=0, knn_tie=0, short_rows=0, maxnn_tie=0, on_r2=0, rows_0=0, rows_1=0,
               rows_small=0, rows_window_m1=0, rows_window=0, rows_window_p1=0, rows_long=0, rows_whole=0)
    if len(Q):
        _, k1 = knn_rows(T, Q, 1)
        out["on_point"] = int((k1[:, 0] == 0).sum())
    for k in ks:
        if k > n:
            out["short_rows"] += len(Q)
        if k >= n:
            continue
        _, key = knn_rows(T, Q, k + 1)
        out["knn_tie"] += int((key[:, k - 1] == key[:, k]).sum())
    for r, max_nn in radii:
        rows = mr.radius_rows(T, Q, r)
        out["on_r2"] += int((rows["out_key"] == rows["r2"]).sum())
        off, idx, key = radius_csr(T, Q, r, 0)
        ln = np.diff(off)
        if max_nn > 0:
            cut = np.flatnonzero(ln > max_nn)
            out["maxnn_tie"] += int(sum(key[off[i] + max_nn - 1] == key[off[i] + max_nn] for i in cut))
            continue
        out["rows_0"] += int((ln == 0).sum())
        out["rows_1"] += int((ln == 1).sum())
        out["rows_small"] += int(((ln >= 2) & (ln < window - 1)).sum())
        out["rows_window_m1"] += int((ln == window - 1).sum())
        out["rows_window"] += int((ln == window).sum())
        out["rows_window_p1"] += int((ln == window + 1).sum())
        out["rows_long"] += int((ln > window).sum())
        out["rows_whole"] += int((ln == n).sum())
    return out
