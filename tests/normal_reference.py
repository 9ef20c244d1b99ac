"""An independent reference for surface normal estimation (rgc_normal_estimate): numpy and scipy only, nothing from oracle/ and nothing from the product.

Neighbours: the search reference's rows (tests/search_reference.py: fp64 cKDTree candidates, the fp32 key ((dx dx + dy dy) + dz dz) recomputed with float32
ufuncs, ascending (key, index), every row PROVEN complete by the margin rule) -- the min(k, n_surface) smallest on the k route, every key < float32(r r),
strict, on the radius route.

Moments: in numpy longdouble about the query q, as the header states them -- d = P - q, S1 = sum d, S2 = sum d d^T, mean = S1 / m, centroid = q + mean,
cov = S2 / m - mean mean^T -- together with the sums of ABSOLUTE terms A1 = sum |d|, A2 = sum |d d^T| from which every tolerance is derived:

  bound_cov[a, b] = (m + 4) 2^-53 (A2[a, b] / m + 2 A1[a] A1[b] / m^2)      any order of an m-term fp64 sum errs by at most (m - 1) u of the sum of absolute
  bound_cen[a]    = (m + 4) 2^-53 (|q[a]| + A1[a] / m)                      terms, u = 2^-53; the products, the division and the final subtraction or addition
                                                                            add one u each (the + 4, with one to spare); the product of the two means carries the
                                                                            error of BOTH sums (the factor 2)
  bound_eig       = |bound_cov|_F (the full symmetric 3 x 3)                Weyl: an eigenvalue moves by at most the perturbation's 2-norm <= its Frobenius norm
  bound_n         = 8 m 2^-53 |A|_F / (l1 - l0) + 2^-24                     A[a, b] = A2[a, b] / m + 2 A1[a] A1[b] / m^2: the sums' rounding through the
                                                                            eigenvector's condition 1 / gap, times 8 for the 3 x 3 Jacobi solver (the form of
                                                                            plane_reference.refine), plus one fp32 rounding of a component of magnitude <= 1
Eigenpairs: numpy.linalg.eigh of the float64 rounding of cov (ascending).  A query is DECIDED when (l1 - l0) / trace >= knn_reference.GAP_MIN.

The sign rules are the header's: flip = 1 negates when ((vx - qx) nx + (vy - qy) ny) + (vz - qz) nz < 0; flip = 0 makes the first component of largest
magnitude positive.  sign_sure says where the rule's outcome cannot depend on an error of bound_n per component.

pcl_point_normal() is a literal restatement, FROM MEMORY, of PCL's fp32 unshifted computePointNormal (computeMeanAndCovarianceMatrix's nine running sums in
float, then the smallest eigenvector): the deviation the header lists, for tests/test_normal_reference.py to demonstrate."""
from __future__ import annotations

import numpy as np

import knn_reference as kr
import search_reference as sr

U = 2.0 ** -53
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))     # the order of out_cov6


def _xyz(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)[:, :3])


def neighbours(queries, surface, k: int = 0, radius: float = 0.0):
    """CSR (off (nq + 1,) int64, idx (m,) int64): the members of every query, ascending (key, index)"""
    Q, T = _xyz(queries), _xyz(surface)
    if (k != 0) == (radius != 0.0):
        raise ValueError("exactly one of k and radius")
    if k:
        m = min(int(k), len(T))
        idx, _ = sr.knn_rows(T, Q, m)
        return np.arange(len(Q) + 1, dtype=np.int64) * m, idx.reshape(-1).astype(np.int64)
    off, idx, _ = sr.radius_csr(T, Q, radius)
    return off.astype(np.int64), idx.astype(np.int64)


def _seg(values, off):
    """per-row sums of values (m, c) over the CSR rows off, in longdouble; an empty row sums to 0"""
    nq = len(off) - 1
    out = np.zeros((nq, values.shape[1]), np.longdouble)
    cnt = np.diff(off)
    rows = np.flatnonzero(cnt > 0)
    if rows.size:
        out[rows] = np.add.reduceat(values, off[rows], axis=0)
    return out


def estimate(queries, surface=None, k: int = 0, radius: float = 0.0, viewpoint=(0.0, 0.0, 0.0), flip: bool = True) -> dict:
    """everything the device is compared with, per query (see the module docstring)"""
    Q = _xyz(queries)
    T = Q if surface is None else _xyz(surface)
    nq = len(Q)
    off, idx = neighbours(Q, T, k, radius)
    m = np.diff(off)
    row = np.repeat(np.arange(nq), m)
    q = Q.astype(np.longdouble)
    d = T[idx].astype(np.longdouble) - q[row]
    prod = np.stack([d[:, a] * d[:, b] for a, b in PAIRS], axis=1)
    S1, S2 = _seg(d, off), _seg(prod, off)
    A1, A2 = _seg(np.abs(d), off), _seg(np.abs(prod), off)
    valid = m >= 3
    mm = np.where(m > 0, m, 1).astype(np.longdouble)[:, None]
    mean = S1 / mm
    cov6 = S2 / mm - np.stack([mean[:, a] * mean[:, b] for a, b in PAIRS], axis=1)
    cen = q + mean
    A6 = (A2 / mm + 2 * np.stack([A1[:, a] * A1[:, b] for a, b in PAIRS], axis=1) / (mm * mm)).astype(np.float64)
    mf = m.astype(np.float64)[:, None]
    bound_cov = (mf + 4) * U * A6
    bound_cen = (mf + 4) * U * (np.abs(Q.astype(np.float64)) + (A1 / mm).astype(np.float64))
    S = np.zeros((nq, 3, 3))
    A33, B33 = np.zeros((nq, 3, 3)), np.zeros((nq, 3, 3))
    for j, (a, b) in enumerate(PAIRS):
        S[:, a, b] = S[:, b, a] = cov6[:, j].astype(np.float64)
        A33[:, a, b] = A33[:, b, a] = A6[:, j]
        B33[:, a, b] = B33[:, b, a] = bound_cov[:, j]
    ev, V = np.linalg.eigh(S)
    trace = np.trace(S, axis1=1, axis2=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap_rel = np.where(trace > 0, (ev[:, 1] - ev[:, 0]) / trace, 0.0)
        bound_n = 8.0 * mf[:, 0] * U * np.sqrt((A33 ** 2).sum(axis=(1, 2))) / (ev[:, 1] - ev[:, 0]) + 2.0 ** -24
        curvature = np.where(trace > 0, np.abs(ev[:, 0]) / trace, 0.0)
    bound_n = np.where(ev[:, 1] - ev[:, 0] > 0, bound_n, np.inf)
    decided = valid & (gap_rel >= kr.GAP_MIN)
    n = V[:, :, 0].copy()
    vp = np.asarray(viewpoint, np.float32).astype(np.float64)
    to_vp = vp[None, :] - Q.astype(np.float64)
    if flip:
        dot = (to_vp[:, 0] * n[:, 0] + to_vp[:, 1] * n[:, 1]) + to_vp[:, 2] * n[:, 2]
        neg = dot < 0
        sign_sure = np.abs(dot) > np.abs(to_vp).sum(axis=1) * bound_n
    else:
        an = np.abs(n)
        big = np.argmax(an, axis=1)                          # (the first of equal maxima)
        neg = np.take_along_axis(n, big[:, None], axis=1)[:, 0] < 0
        srt = np.sort(an, axis=1)
        sign_sure = (srt[:, 2] - srt[:, 1] > 2 * bound_n) & (srt[:, 2] > bound_n)
    n[neg] = -n[neg]
    return dict(count=m.astype(np.int32), valid=valid, n_valid=int(valid.sum()), off=off, idx=idx, cov6=cov6.astype(np.float64), centroid=cen.astype(np.float64), S=S,
                bound_cov=bound_cov, bound_cen=bound_cen, bound_eig=np.sqrt((B33 ** 2).sum(axis=(1, 2))), ev=ev, trace=trace, curvature=curvature, gap_rel=gap_rel,
                decided=decided, normal=n, bound_n=bound_n, sign_sure=sign_sure & decided)


def pcl_point_normal(queries, surface, off, idx):
    """PCL's computePointNormal on the rows (off, idx), restated from memory [3P-memory: common/impl/centroid.hpp, computeMeanAndCovarianceMatrix with Scalar =
    float; features/normal_3d.h, solvePlaneParameters]: nine float32 running sums of the UNSHIFTED coordinates in row order, accu /= m, cov = accu - mean
    mean^T in float32, the eigenvector of the smallest eigenvalue.  (nq, 3) float64 unit normals, sign undefined; NaN where m < 3"""
    T = _xyz(surface)
    nq = len(off) - 1
    out = np.full((nq, 3), np.nan)
    for i in range(nq):
        P = T[idx[off[i]:off[i + 1]]]
        if len(P) < 3:
            continue
        accu = np.zeros(9, np.float32)
        for p in P:
            x, y, z = p
            accu += np.array([x * x, x * y, x * z, y * y, y * z, z * z, x, y, z], np.float32)
        accu /= np.float32(len(P))
        mx, my, mz = accu[6:]
        C = np.array([[accu[0] - mx * mx, accu[1] - mx * my, accu[2] - mx * mz],
                      [accu[1] - mx * my, accu[3] - my * my, accu[4] - my * mz],
                      [accu[2] - mx * mz, accu[4] - my * mz, accu[5] - mz * mz]], np.float32)
        out[i] = np.linalg.eigh(C.astype(np.float64))[1][:, 0]
    return out
