"""FastGICPMultiPoints in numpy, fp64: an independent reference for the rgc_gicpmp_* entry points, restated from the text of fast_gicp::FastGICPMultiPoints
(include/fast_gicp/gicp/experimental/fast_gicp_mp_impl.hpp:92-221).  Imports nothing from oracle/ and nothing from the product.

Neighbours (:145): the fp32 query ((m0 x + m1 y) + m2 z) + m3, the fp32 key ((dx dx + dy dy) + dz dz), a member iff key < r2, strict, with
r2 = float32(float64(r) * float64(r)) (pcl::KdTreeFLANN::radiusSearch).  Candidates come from an fp64 cKDTree ball of a LARGER radius; their keys are
recomputed with float32 ufuncs and the strict rule applied; a row is complete because the superset radius exceeds what any member's true distance
can be (radius_rows asserts the inequality, and that no member lies near the superset's edge).
Weights (:184-185): w = max(1e-3, min(1, 1 - float64(float32(sqrt(float64(key)))) / r)) -- the correctly rounded fp32 root.
Merge (:180-195), fp64, the reference's casts to fp32 not made: sw = sum w, mean_B = sum w b / sw, cov_B = sum w C_B / sw.
Terms (:197-213): a = R p + t, d = mean_B - a, M = (cov_B + R C_A R^T)^-1, loss l = M d, J = M [skew(a) | -I]; plain Gauss-Newton over those rows:
cost = sum l.l, H = sum J^T J, b = sum J^T l (W = M M).  Driver (:92-108) with the update T <- [so3_exp(d_r) | d_t] T (ndt_reference.increment) and
the convergence test of :118-127 after the update.  The covariances are GIVEN."""
import numpy as np
from scipy.spatial import cKDTree

import nn_reference as nn
from gicp_reference import adjugate_inverse, ordered_sum  # noqa: F401  (re-exported for the tests)
from ndt_reference import increment, skew

U = 2.0 ** -53


def r2_of(r):
    return np.float32(float(r) * float(r))


def fp32_keys(q, b):
    """((dx dx + dy dy) + dz dz) with float32 ufuncs, row by row"""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    d = q - b
    dd = d * d
    return ((dd[:, 0] + dd[:, 1]) + dd[:, 2]).astype(np.float32)


def weights(key, r):
    root = np.sqrt(np.asarray(key, np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)
    raw = 1.0 - root / float(r)
    return np.maximum(1e-3, np.minimum(1.0, raw)), raw


def radius_rows(target, queries, r):
    """CSR rows of every query: dict(off (nq + 1,) int64, row (m,) int64, idx (m,) int64 ascending inside a row, key (m,) float32) and, for the census,
    the keys of the superset's candidates that are NOT members (out_key)"""
    T = np.ascontiguousarray(np.asarray(target, np.float32)[:, :3])
    Q = np.ascontiguousarray(np.asarray(queries, np.float32)[:, :3])
    r2 = r2_of(r)
    big = max(float(np.abs(T).max(initial=0)), float(np.abs(Q).max(initial=0)), 1.0)
    margin = 16.0 * float(np.spacing(np.float32(big)))
    # a member's key < r2; the key's five roundings and the three differences' move it by at most 8 * 2^-24 relative, so its true distance is
    # below sqrt(r2) (1 + 8 * 2^-24); the superset's radius leaves that and the margin behind
    reach = float(np.sqrt(np.float64(r2))) * (1.0 + 8 * 2.0 ** -24)
    sup = reach * (1.0 + 1e-5) + 2 * margin
    assert sup > reach + margin
    T64, Q64 = T.astype(np.float64), Q.astype(np.float64)
    lists = cKDTree(T64).query_ball_point(Q64, sup, return_sorted=True)      # ascending index inside a row
    cnt = np.fromiter((len(l) for l in lists), np.int64, len(lists))
    row = np.repeat(np.arange(len(Q)), cnt)
    cand = np.concatenate([np.asarray(l, np.int64) for l in lists]) if cnt.sum() else np.zeros(0, np.int64)
    key = fp32_keys(Q[row], T[cand])
    inside = key < r2
    d64 = np.linalg.norm(Q64[row[inside]] - T64[cand[inside]], axis=1)
    assert d64.size == 0 or d64.max() < sup - margin, "a member near the superset's edge: the rows are not proven complete"
    row_in, idx_in, key_in = row[inside], cand[inside], key[inside]
    off = np.concatenate([[0], np.cumsum(np.bincount(row_in, minlength=len(Q)))]).astype(np.int64)
    return dict(off=off, row=row_in, idx=idx_in, key=key_in, out_key=key[~inside], r2=r2)


def _seg_sum(row, values, n, descending):
    """per-row sequential sums (bincount adds in array order), first to last or last to first"""
    values = np.asarray(values, np.float64)
    if descending:
        row, values = row[::-1], values[::-1]
    if values.ndim == 1:
        return np.bincount(row, values, minlength=n)
    return np.stack([np.bincount(row, values[:, a], minlength=n) for a in range(values.shape[1])], axis=1)


def cov6_of(C):
    C = np.asarray(C, np.float64).reshape(-1, 3, 3)
    return np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], axis=1)


def cov33_of(c6):
    C = np.empty((len(c6), 3, 3))
    C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2] = c6.T
    C[:, 1, 0], C[:, 2, 0], C[:, 2, 1] = C[:, 0, 1], C[:, 0, 2], C[:, 1, 2]
    return C


class GICPMP:
    def __init__(self, radius=0.5):
        self.r = float(radius)
        self.source = self.target = self.cov_s = self.cov_t = None
        self.last = None

    def set_target(self, pts, cov):
        self.target, self.cov_t = np.asarray(pts, np.float32)[:, :3], np.asarray(cov, np.float64).reshape(-1, 3, 3)
        assert len(self.target) == len(self.cov_t)

    def set_source(self, pts, cov):
        self.source, self.cov_s = np.asarray(pts, np.float32)[:, :3], np.asarray(cov, np.float64).reshape(-1, 3, 3)
        assert len(self.source) == len(self.cov_s)

    def rows(self, T):
        q = nn.transform_f32(self.source, np.asarray(T, np.float64).astype(np.float32))
        return radius_rows(self.target, q, self.r)

    def merge(self, T, descending=False, rows=None):
        """dict(count, sw, mean (n, 3), cov6 (n, 6), and the bounds' sums abs_mean (n, 3) = sum w |b| / sw, abs_cov6 = sum w |C| / sw, rows)"""
        rw = self.rows(T) if rows is None else rows
        n = len(self.source)
        row, idx = rw["row"], rw["idx"]
        w, raw = weights(rw["key"], self.r)
        b, c6 = self.target[idx].astype(np.float64), cov6_of(self.cov_t[idx])
        count = np.bincount(row, minlength=n)
        sw = _seg_sum(row, w, n, descending)
        has = count > 0
        den = np.where(has, sw, 1.0)
        mean = _seg_sum(row, w[:, None] * b, n, descending) / den[:, None]
        cov6 = _seg_sum(row, w[:, None] * c6, n, descending) / den[:, None]
        abs_mean = _seg_sum(row, w[:, None] * np.abs(b), n, descending) / den[:, None]
        abs_cov6 = _seg_sum(row, w[:, None] * np.abs(c6), n, descending) / den[:, None]
        return dict(count=count, sw=sw, mean=mean, cov6=cov6, abs_mean=abs_mean, abs_cov6=abs_cov6, rows=rw, w=w, raw=raw)

    def loss_rows(self, T, merged, inverse=np.linalg.inv, M=None):
        """per source point with a neighbour: (i, loss (m, 3), J (m, 3, 6), M); M given: frozen"""
        T = np.asarray(T, np.float64)
        i = np.flatnonzero(merged["count"] > 0)
        R, t = T[:3, :3], T[:3, 3]
        a = self.source[i].astype(np.float64) @ R.T + t
        d = merged["mean"][i] - a
        if M is None:
            S = cov33_of(merged["cov6"][i]) + R @ self.cov_s[i] @ R.T
            M = inverse(S) if len(i) else np.zeros((0, 3, 3))
        D = np.concatenate([skew(a), -np.broadcast_to(np.eye(3), (len(a), 3, 3))], axis=2)
        return i, np.einsum("nij,nj->ni", M, d), np.einsum("nij,njb->nib", M, D), M

    def linearize(self, T, descending=False, inverse=np.linalg.inv):
        """returns cost, H, b; self.last = the merge"""
        T = np.asarray(T, np.float64)
        m = self.merge(T, descending)
        self.last = m
        _, l, J, _ = self.loss_rows(T, m, inverse)
        return (float(ordered_sum(np.einsum("ni,ni->n", l, l), descending)), ordered_sum(np.einsum("nia,nib->nab", J, J), descending),
                ordered_sum(np.einsum("nia,ni->na", J, l), descending))

    def num_points(self):
        return int((self.last["count"] > 0).sum())

    def num_pairs(self):
        return int(self.last["count"].sum())

    def align(self, guess, max_iterations=64, rotation_epsilon=1e-5, transformation_epsilon=1e-5, perturb=0.0):
        """:92-108 -- returns T (fp64), iterations (linearisations made), converged, failed, the H of the last step taken"""
        x0 = np.asarray(guess, np.float32).astype(np.float64).copy()
        x0[3] = [0, 0, 0, 1]
        x0[:3, 3] += perturb
        conv, failed, iters, Hfin = False, False, 0, np.eye(6)
        for it in range(max_iterations):
            iters = it + 1
            _, H, b = self.linearize(x0)
            if self.num_points() == 0:
                failed = True
                break
            try:
                d = np.linalg.solve(H, -b)
            except np.linalg.LinAlgError:
                failed = True
                break
            xi, delta = increment(d, x0)
            if not (np.isfinite(d).all() and np.isfinite(xi).all()):
                failed = True
                break
            x0, Hfin = xi, H
            if max(np.abs(delta[:3, :3] - np.eye(3)).max() / rotation_epsilon, np.abs(delta[:3, 3]).max() / transformation_epsilon) < 1:
                conv = True
                break
        return x0, iters, conv, failed, Hfin


def literal_linearize(source, cov_s, target, cov_t, T, r):
    """fast_gicp_mp_impl.hpp:130-221 point by point with the reference's 4x4 matrices: homogeneous 4-vectors (w = 1), covariances padded with a zero row and
    column, RCR = cov_B + trans cov_A trans^T with RCR(3,3) = 1, the full 4x4 inverse, the 4x6 dtdx0, losses RCRd.head<3>() and rows jlossexp.block<3,6>;
    then the Gauss-Newton sums over those rows.  fp64 throughout (the casts to fp32 of :194-195 are not made).  Returns cost, H, b, kept."""
    T = np.asarray(T, np.float64)
    src, tgt = np.asarray(source, np.float32)[:, :3], np.asarray(target, np.float32)[:, :3]
    rw = radius_rows(tgt, nn.transform_f32(src, T.astype(np.float32)), r)
    cost, H, b, kept = 0.0, np.zeros((6, 6)), np.zeros(6), 0
    for i in range(len(src)):
        k_indices, k_sq = rw["idx"][rw["off"][i]:rw["off"][i + 1]], rw["key"][rw["off"][i]:rw["off"][i + 1]]
        if len(k_indices) == 0:                                                        # :176
            continue
        sum_w, sum_mean_B, sum_cov_B = 0.0, np.zeros(4), np.zeros((4, 4))
        for j, k2 in zip(k_indices, k_sq):                                             # :183-192
            w = 1 - float(np.float32(np.sqrt(np.float64(k2)))) / r
            w = max(1e-3, min(1.0, w))
            sum_w += w
            cB = np.zeros((4, 4))
            cB[:3, :3] = cov_t[j]
            sum_mean_B += w * np.append(tgt[j].astype(np.float64), 1.0)
            sum_cov_B += w * cB
        mean_B, cov_B = sum_mean_B / sum_w, sum_cov_B / sum_w                          # :194-195
        cA = np.zeros((4, 4))
        cA[:3, :3] = cov_s[i]
        transed = T @ np.append(src[i].astype(np.float64), 1.0)                        # :197
        d = mean_B - transed
        RCR = cov_B + T @ cA @ T.T
        RCR[3, 3] = 1.0                                                                # :200
        RCR_inv = np.linalg.inv(RCR)
        RCRd = RCR_inv @ d
        dtdx0 = np.zeros((4, 6))
        dtdx0[:3, :3] = skew(transed[:3])
        dtdx0[:3, 3:] = -np.eye(3)
        jl = (RCR_inv @ dtdx0)[:3]
        l = RCRd[:3]
        cost += float(l @ l)
        H += jl.T @ jl
        b += jl.T @ l
        kept += 1
    return cost, H, b, kept


def census(rw, r):
    """what a case's rows hold: queries by neighbour count, members by weight, keys on and next to the gate"""
    cnt = np.diff(rw["off"])
    w, raw = weights(rw["key"], r)
    r2 = rw["r2"]
    allk = np.concatenate([rw["key"], rw["out_key"]])
    return dict(q0=int((cnt == 0).sum()), q1=int((cnt == 1).sum()), q2_63=int(((cnt >= 2) & (cnt <= 63)).sum()), q64=int((cnt >= 64).sum()),
                clamped=int((raw < 1e-3).sum()), w_one=int((w == 1.0).sum()), on_r2=int((allk == r2).sum()),
                step_inside=int((allk == np.nextafter(r2, np.float32(0))).sum()), step_outside=int((allk == np.nextafter(r2, np.float32(np.inf))).sum()),
                pairs=int(cnt.sum()), max_row=int(cnt.max(initial=0)))
