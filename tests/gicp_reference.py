"""FastGICP in numpy, fp64: an independent reference for the rgc_gicp_* entry points, restated from the formulas of fast_gicp::FastGICP
(include/fast_gicp/gicp/impl/fast_gicp_impl.hpp:115-237) and LsqRegistration's driver (lsq_registration_impl.hpp:53-172).  Imports nothing from oracle/.

Correspondences are nn_reference.nearest(target, transform_f32(source, float32(T))): the fp32 query, the fp32 key ((dx dx + dy dy) + dz dz), ties to
the smaller index; a pair is kept iff float64(key) < d_max * d_max (:136, strict).  Everything after that is fp64: a = R p + t, e = b_j - a,
M = (C_B[j] + R C_A[i] R^T)^-1 (3x3), cost = sum e^T M e, J = [skew(a), -I], H = sum J^T M J, b = sum J^T M e.  compute_error re-uses the pairs and
the M of the last linearize.  The covariances are GIVEN (the product's own, from its getters, in the GPU tests): this file has a plain kNN covariance
of its own (knn_covariances) only so that the CPU tests have something to feed it."""
import numpy as np

import nn_reference as nn
from ndt_reference import increment, skew

FLT_MAX = float(np.finfo(np.float32).max)


def adjugate_inverse(S):
    """inverse of a stack of symmetric 3x3 by the adjugate (the other way to the same matrix: numpy.linalg.inv is LU with pivoting)"""
    a, b, c, d, e, f = S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    det = a * c00 + b * c01 + c * c02
    M = np.empty_like(S)
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2] = c00 / det, c01 / det, c02 / det
    M[:, 1, 1], M[:, 1, 2], M[:, 2, 2] = (a * f - c * c) / det, (b * c - a * e) / det, (a * d - b * b) / det
    M[:, 1, 0], M[:, 2, 0], M[:, 2, 1] = M[:, 0, 1], M[:, 0, 2], M[:, 1, 2]
    return M


def ordered_sum(x, descending=False):
    """strictly sequential sum over axis 0, first to last or last to first (cumsum adds one term at a time)"""
    x = np.asarray(x, np.float64)
    if len(x) == 0:
        return np.zeros(x.shape[1:])
    return np.cumsum(x[::-1] if descending else x, axis=0)[-1]


def knn_covariances(points, k=20):
    """PLANE-regularised covariance of the k nearest neighbours (the point itself included) of every point: eigenvalues (1e-3, 1, 1)
    (fast_gicp_impl.hpp:241-298).  (n, 3, 3) fp64."""
    P = np.asarray(points, np.float32)[:, :3]
    idx, _ = nn.nearest_k(P, P, k)
    nb = P.astype(np.float64)[idx]
    d = nb - nb.mean(axis=1, keepdims=True)
    cov = np.einsum("nki,nkj->nij", d, d) / (k - 1)
    _, V = np.linalg.eigh(cov)
    return np.einsum("nia,a,nja->nij", V, np.array([1e-3, 1.0, 1.0]), V)


class GICP:
    def __init__(self, d_max=FLT_MAX):
        self.d_max = float(d_max)
        self.source = self.target = self.cov_s = self.cov_t = None
        self.corr = None        # (idx (ns,) int64 with -1 where rejected, key (ns,) float32, M (kept, 3, 3))

    def set_target(self, pts, cov):
        self.target, self.cov_t, self.corr = np.asarray(pts, np.float32)[:, :3], np.asarray(cov, np.float64).reshape(-1, 3, 3), None
        assert len(self.target) == len(self.cov_t)

    def set_source(self, pts, cov):
        self.source, self.cov_s, self.corr = np.asarray(pts, np.float32)[:, :3], np.asarray(cov, np.float64).reshape(-1, 3, 3), None
        assert len(self.source) == len(self.cov_s)

    def correspondences(self, T):
        """(idx, key) at T: idx -1 where rejected, key kept either way (:135-136)"""
        q = nn.transform_f32(self.source, np.asarray(T, np.float64).astype(np.float32))
        j, key = nn.nearest(self.target, q)
        keep = key.astype(np.float64) < self.d_max * self.d_max
        return np.where(keep, j, -1), key

    def _terms(self, T):
        idx, _, M = self.corr
        i = np.flatnonzero(idx >= 0)
        R, t = T[:3, :3], T[:3, 3]
        a = self.source[i].astype(np.float64) @ R.T + t
        e = self.target[idx[i]].astype(np.float64) - a
        Me = np.einsum("nij,nj->ni", M, e)
        J = np.concatenate([skew(a), -np.broadcast_to(np.eye(3), (len(a), 3, 3))], axis=2)
        return np.einsum("ni,ni->n", e, Me), np.einsum("nia,nij,njb->nab", J, M, J), np.einsum("nia,ni->na", J, Me)

    def linearize(self, T, descending=False, inverse=np.linalg.inv):
        """update_correspondences + linearize (:115-211): returns cost, H, b"""
        T = np.asarray(T, np.float64)
        idx, key = self.correspondences(T)
        i = np.flatnonzero(idx >= 0)
        R = T[:3, :3]
        S = self.cov_t[idx[i]] + R @ self.cov_s[i] @ R.T
        M = inverse(S) if len(i) else np.zeros((0, 3, 3))
        self.corr = (idx, key, M)
        c, H, b = self._terms(T)
        return float(ordered_sum(c, descending)), ordered_sum(H, descending), ordered_sum(b, descending)

    def num_kept(self):
        return int((self.corr[0] >= 0).sum())

    def compute_error(self, T, descending=False):
        """the frozen cost (:214-237)"""
        return float(ordered_sum(self._terms(np.asarray(T, np.float64))[0], descending))

    def align(self, guess, max_iterations=64, lm_max_iterations=10, rotation_eps=2e-3, translation_eps=5e-4, init_lambda_factor=1e-9, perturb=0.0):
        """LsqRegistration::computeTransformation (lsq_registration_impl.hpp:53-79) with step_lm (:125-172), as ndt_reference.NDT.align restates it:
        returns T (fp64), iterations, converged, lm_failed, final Hessian.  perturb: added to the translation of the guess after its cast to fp32 (how far
        two solves from all but the same guess end apart is the margin a comparison of poses is entitled to)"""
        def is_converged(delta):
            m = max(np.abs(delta[:3, :3] - np.eye(3)).max() / rotation_eps, np.abs(delta[:3, 3]).max() / translation_eps)
            return m < 1
        x0 = np.asarray(guess, np.float32).astype(np.float64).copy()
        x0[3] = [0, 0, 0, 1]
        x0[:3, 3] += perturb
        lam, conv, failed, iters, Hfin = -1.0, False, False, 0, np.eye(6)
        for it in range(max_iterations):
            if conv:
                break
            iters = it + 1
            y0, H, b = self.linearize(x0)
            if lam < 0:
                lam = init_lambda_factor * np.abs(np.diag(H)).max()
            nu, ok, delta = 2.0, False, np.zeros((4, 4))
            for _ in range(lm_max_iterations):
                d = np.linalg.solve(H + lam * np.eye(6), -b)
                xi, delta = increment(d, x0)
                yi = self.compute_error(xi)
                rho = (y0 - yi) / float(d @ (lam * d - b))
                if rho < 0:
                    if is_converged(delta):
                        ok = True
                        break
                    lam, nu = nu * lam, 2 * nu
                    continue
                x0, lam, Hfin, ok = xi, lam * max(1.0 / 3.0, 1 - (2 * rho - 1) ** 3), H, True
                break
            if not ok:
                failed = True
                break
            conv = is_converged(delta)
        return x0, iters, conv, failed, Hfin


def literal_linearize(source, cov_s, target, cov_t, T, d_max=FLT_MAX):
    """fast_gicp_impl.hpp:115-211 point by point, with the reference's 4x4 matrices: covariances padded with a zero row and column, RCR = cov_B + T cov_A
    T^T with RCR(3,3) = 1, the full 4x4 inverse, M(3,3) = 0, 4-vectors with w = 1, the 4x6 Jacobian.  Returns cost, H, b."""
    T = np.asarray(T, np.float64)
    src, tgt = np.asarray(source, np.float32)[:, :3], np.asarray(target, np.float32)[:, :3]
    q = nn.transform_f32(src, T.astype(np.float32))
    j, key = nn.nearest(tgt, q)
    cost, H, b = 0.0, np.zeros((6, 6)), np.zeros(6)
    for i in range(len(src)):
        if not float(key[i]) < d_max * d_max:
            continue
        cA, cB = np.zeros((4, 4)), np.zeros((4, 4))
        cA[:3, :3], cB[:3, :3] = cov_s[i], cov_t[j[i]]
        RCR = cB + T @ cA @ T.T
        RCR[3, 3] = 1.0
        M = np.linalg.inv(RCR)
        M[3, 3] = 0.0
        mean_A = np.append(src[i].astype(np.float64), 1.0)
        mean_B = np.append(tgt[j[i]].astype(np.float64), 1.0)
        a = T @ mean_A
        e = mean_B - a
        cost += float(e @ M @ e)
        J = np.zeros((4, 6))
        J[:3, :3] = skew(a[:3])
        J[:3, 3:] = -np.eye(3)
        H += J.T @ M @ J
        b += J.T @ M @ e
    return cost, H, b
