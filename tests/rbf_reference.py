"""An independent reference for RBF-kernel covariance estimation (numpy and scipy only; nothing from oracle/): rgc_set_covariance_estimation(RGC_COV_RBF),
the reference's GPU_RBF_KERNEL (src/fast_gicp/cuda/covariance_estimation_rbf.cu:59-151).

Semantics (include/rgc_hip.h).  The ball of point i is ``{ j : key(i, j) <= max_dist_sq }`` with the product's fp32 key ``((dx*dx + dy*dy) + dz*dz)``
(``knn_reference.fp32_keys``) and ``max_dist_sq = float32(max_dist) * float32(max_dist)``; ``w_j = exp(-float32(kernel_width) * key)``,
``d_j = P_j - P_i``, ``S0 = sum w``, ``S1 = sum w d``, ``S2 = sum w d d^T``, ``m = S1 / S0``, ``cov = S2 / S0 - m m^T``, then the RegularizationMethod.

Here the candidates come from an fp64 ``cKDTree.query_ball_point`` at ``max_dist`` plus a margin of a few fp32 ulps of the largest coordinate (an fp32 key
differs from the exact squared distance by a few relative ulps: nothing whose key can round onto ``max_dist_sq`` lies outside), membership is decided by
the fp32 keys, and the moments are summed in ``np.longdouble`` centred on the query (64-bit mantissa on x86: its own error is 2^-11 of the bound below).

``literal`` restates covariance_estimation_rbf.cu as it is written -- blocks of 512 candidates, one partial {sum w, sum w p, sum w p p^T} per (point,
block) around the ORIGIN, the partials added block by block, finalize() -- in longdouble and WITHOUT the padding points (the reference's padding defect,
INTEGRATION.md §4).  tests/test_rbf_reference.py holds the two forms equal.

THE BAR FOR NONE (derived, not measured).  u = 2^-53.  One entry (a, b) of the covariance is S2_ab / S0 - (S1_a / S0)(S1_b / S0).  To first order:
  * a sum of m terms t_j accumulated one by one has an error of at most (m - 1) u sum|t_j|; every term carries exp's error (about 1 ulp of w_j) and its
    own roundings (w * d_a, * d_b, and the conversion of the key's product: 3 at most): (m + 3) u sum|t_j| for each of S0, S1_a, S2_ab, and the division
    and the subtraction that follow add less than 3 u of the same size: (m + 8) u sum|t_j| covers a sum and what is done with it;
  * S2_ab / S0 therefore errs by (m + 8) u (T2_ab + T2_ab) / S0, T2_ab = sum w |d_a d_b| (once for S2's terms, once for S0's: |S2_ab| <= T2_ab and S0's
    terms are all positive);
  * S1_a / S0 errs by (m + 8) u 2 A_a / S0, A_a = sum w |d_a|, and |S1_a / S0| <= A_a / S0: the product of the two means errs by (m + 8) u 4 A_a A_b / S0^2.
So |gpu - ref| <= (m + 8) u ``abs_terms`` / S0 with ``abs_terms[a, b] = 2 T2_ab + 4 A_a A_b / S0``: the sum of the absolute values of every term that
enters the entry, each counted for every sum whose rounding it is subject to.  ``bound_none`` returns that matrix.

THE BAR FOR THE EIGEN-BASED METHODS.  The same bound matrix B, propagated through the eigen-decomposition: an eigenvector turns by at most ||B||_F / gap
and the regularised matrix U diag(values) U^T moves by at most 4 max(values) ||B||_F / gap: 2 max(values) ||B||_F / gap for the two factors U, each
turned, and as much again for the values themselves, which follow the eigenvalues (MIN_EIG: by ||B||_F at most, and gap <= max(values) / 2;
NORMALIZED_MIN_EIG: by 2 ||B||_F / l1, and gap <= l1 / 2), the second order and eigh's own error.  gap = the smallest difference between eigenvalues the method must tell apart (PLANE: l2 - l3, the normal's; MIN_EIG and
NORMALIZED_MIN_EIG: both gaps, every eigenvalue keeps its own direction).  Rows with gap < 1e-6 trace are left out (``GAP_MIN``).  FROBENIUS has no
eigenvectors: C = ||(S + 1e-3 I)^-1||_F (S + 1e-3 I), whose sensitivity to S is the condition number of S + 1e-3 I: B scaled by it (times
||(S + 1e-3 I)^-1||_F, the size C has relative to S, and 2 for the two places S enters).
"""
from __future__ import annotations

import numpy as np
from scipy.spatial import cKDTree

from knn_reference import fp32_keys

U = 2.0 ** -53
GAP_MIN = 1e-6
METHODS = ("NONE", "MIN_EIG", "NORMALIZED_MIN_EIG", "PLANE", "FROBENIUS")     # rgc_regularization_method's order
TRI = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
LD = np.longdouble


def effective_max_dist(kernel_width: float, max_dist: float) -> float:
    """fast_vgicp_cuda_impl.hpp:46-51"""
    return 5.0 * kernel_width if max_dist <= 0 else max_dist


def balls(xyz, max_dist: float):
    """per point the sorted indices of its ball, decided by the fp32 key (the point itself included)"""
    P = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
    P64 = P.astype(np.float64)
    md = np.float32(max_dist)
    md2 = md * md                                                           # float32 product
    margin = 16.0 * float(np.spacing(np.float32(max(float(np.abs(P).max(initial=0.0)), 1.0))))
    r = float(md) * (1.0 + 2.0 ** -20) + margin if np.isfinite(md2) else np.inf
    cand = cKDTree(P64).query_ball_point(P64, r if np.isfinite(r) else 1e300)
    out = []
    for i, c in enumerate(cand):
        c = np.sort(np.asarray(c, np.int64))
        key = fp32_keys(P, np.array([i]), c[None, :])[0]
        keep = key <= md2
        out.append((c[keep], key[keep]))
    return P, out


def moments(xyz, kernel_width: float, max_dist: float):
    """dict: cov (n, 3, 3) float64 -- the NONE covariance --, m (n,) ball sizes, S0 (n,), abs_terms (n, 3, 3) (see the module text), eig (n, 3) ascending
    eigenvalues of cov, on_radius (n,) members with key == max_dist_sq"""
    md = effective_max_dist(kernel_width, max_dist)
    P, B = balls(xyz, md)
    n = len(P)
    kw = LD(np.float32(kernel_width))
    md2 = np.float32(md) * np.float32(md)
    cov = np.zeros((n, 3, 3)); m = np.zeros(n, np.int64); S0 = np.zeros(n); T = np.zeros((n, 3, 3)); on = np.zeros(n, np.int64)
    PL = P.astype(LD)
    for i, (idx, key) in enumerate(B):
        w = np.exp(-kw * key.astype(LD))
        d = PL[idx] - PL[i]
        s0 = w.sum()
        s1 = (w[:, None] * d).sum(axis=0)
        s2 = np.einsum("j,ja,jb->ab", w, d, d)
        mu = s1 / s0
        cov[i] = (s2 / s0 - np.outer(mu, mu)).astype(np.float64)
        A = (w[:, None] * np.abs(d)).sum(axis=0)
        T[i] = (2 * np.einsum("j,ja,jb->ab", w, np.abs(d), np.abs(d)) + 4 * np.outer(A, A) / s0).astype(np.float64)
        m[i], S0[i], on[i] = len(idx), float(s0), int(np.sum(key == md2))
    return {"cov": cov, "m": m, "S0": S0, "abs_terms": T, "eig": np.linalg.eigvalsh(cov), "on_radius": on}


def literal(xyz, kernel_width: float, max_dist: float, block: int = 512) -> np.ndarray:
    """covariance_estimation_rbf.cu:59-151 as written (blocks of `block` candidates, sums around the origin, the partials of a point added block by block,
    finalize) in longdouble, without the padding points; (n, 3, 3) float64"""
    md = effective_max_dist(kernel_width, max_dist)
    P = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
    n = len(P)
    kw = LD(np.float32(kernel_width))
    md2 = np.float32(md) * np.float32(md)
    PL = P.astype(LD)
    sw = np.zeros(n, LD); sp = np.zeros((n, 3), LD); spp = np.zeros((n, 3, 3), LD)
    q = np.arange(n)
    for b0 in range(0, n, block):
        c = np.arange(b0, min(b0 + block, n))
        key = fp32_keys(P, q, np.broadcast_to(c, (n, len(c))))               # sq_d, :75
        w = np.where(key > md2, LD(0), np.exp(-kw * key.astype(LD)))         # :76-80 (a skipped candidate adds nothing)
        sw += w.sum(axis=1)                                                   # accumulate, :40-44, then operator+=, :33-38
        sp += w @ PL[c]
        spp += np.einsum("qj,ja,jb->qab", w, PL[c], PL[c])
    mean = sp / sw[:, None]                                                   # finalize, :46-52
    cov = (spp - mean[:, :, None] * sp[:, None, :]) / sw[:, None, None]
    return cov.astype(np.float64)


def regularize(S, method: str) -> np.ndarray:
    """fast_gicp_impl.hpp:262-293 (fast_vgicp_cuda.cu:210,218) for all five methods, with eigh"""
    S = np.asarray(S, np.float64)
    if method == "NONE":
        return S.copy()
    if method == "FROBENIUS":
        R = S + 1e-3 * np.eye(3)
        Ci = np.linalg.inv(R)
        return np.linalg.norm(Ci, axis=(1, 2))[:, None, None] * R
    w, V = np.linalg.eigh(S)                                                  # ascending
    if method == "PLANE":
        vals = np.broadcast_to(np.array([1e-3, 1.0, 1.0]), w.shape)
    elif method == "MIN_EIG":
        vals = np.maximum(w, 1e-3)
    elif method == "NORMALIZED_MIN_EIG":
        with np.errstate(invalid="ignore", divide="ignore"):
            t = w / w[:, 2:3]
        vals = np.where(t > 1e-3, t, 1e-3)                                    # (the floor where the quotient is 0 / 0: a zero moment)
    else:
        raise ValueError(method)
    return np.einsum("nij,nj,nkj->nik", V, vals, V)


def bound_none(mom) -> np.ndarray:
    """(n, 3, 3): (m + 8) u abs_terms / S0"""
    return ((mom["m"] + 8) * U / mom["S0"])[:, None, None] * mom["abs_terms"]


def bound(mom, method: str):
    """(bound (n, 3, 3) or (n, 1, 1), compared (n,) bool): the bar of `method` per entry and the rows it applies to"""
    B = bound_none(mom)
    n = len(B)
    if method == "NONE":
        return B, np.ones(n, bool)
    S = mom["cov"]
    nB = np.linalg.norm(B, axis=(1, 2))
    if method == "FROBENIUS":
        R = S + 1e-3 * np.eye(3)
        return (2.0 * np.linalg.cond(R) * np.linalg.norm(np.linalg.inv(R), axis=(1, 2)) * nB)[:, None, None] + 0 * B, np.ones(n, bool)
    w = mom["eig"]
    tr = w.sum(axis=1)
    gap = w[:, 1] - w[:, 0] if method == "PLANE" else np.minimum(w[:, 1] - w[:, 0], w[:, 2] - w[:, 1])
    ok = gap >= GAP_MIN * tr
    ok &= tr > 0
    if method == "PLANE":
        vmax = np.ones(n)
    elif method == "MIN_EIG":
        vmax = np.maximum(w[:, 2], 1e-3)
    else:
        vmax = np.ones(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        b = 4.0 * vmax * nB / gap
    return np.where(ok, b, np.inf)[:, None, None] + 0 * B, ok
