"""FastGICPSingleThread in numpy: an independent reference for the rgc_gicpst_* entry points, restated from fast_gicp::FastGICPSingleThread
(include/fast_gicp/gicp/impl/fast_gicp_st_impl.hpp:19-125).  numpy only; imports nn_reference (the fp32 query) and gicp_reference (the shared term and
LsqRegistration's driver); nothing from oracle/ or the product.

State per source point: corr, key1, key2 (fp32), the anchor (3 fp32), M (3x3 fp64), and whether the last linearisation searched it.  For a pose T:
  q = nn_reference.transform_f32(source, float32(T)) (:44).
  With an anchor a (:46-54): d2 = (dx dx + dy dy) + dz dz of q - a in fp32, d = float64(float32(sqrt(float64(d2)))), max_first =
float64(float32(sqrt(float64(key1)))) + d, min_second = float64(float32(sqrt(float64(key2)))) - d; SKIPPED iff max_first < min_second (strict, fp64):
everything the point has stays.
  Otherwise SEARCHED (:56-75): the two nearest by BRUTE FORCE over the whole target under (key, index) -- key = (dx dx + dy dy) + dz dz with float32
ufuncs; key1 and its index j (ties: the smaller index), key2 = the second smallest key of the multiset (+inf for a target of one point); corr = j
iff float64(key1) < d_max^2 (strict) else -1; anchor = q; for a kept pair M = (C_B[j] + R C_A[i] R^T)^-1 at this pose.
  Terms (:80-120): gicp_reference's term for every pair with corr >= 0 under the stored M.  compute_error: the cost of the state as it is.
`Literal` restates :25-120 point by point with the reference's 4x4 matrices, as a second statement of the same thing."""
import numpy as np

import gicp_reference as gr
import nn_reference as nn
from ndt_reference import skew

FLT_MAX = gr.FLT_MAX


def keys_f32(q, pts):
    """(len(q), len(pts)) float32: (dx dx + dy dy) + dz dz, every operation rounded to fp32"""
    q, pts = np.asarray(q, np.float32), np.asarray(pts, np.float32)
    dx, dy, dz = (q[:, None, a] - pts[None, :, a] for a in range(3))
    return (dx * dx + dy * dy) + dz * dz


def two_nearest(target, q, chunk=256):
    """(j (nq,) int64, key1, key2 (nq,) float32) by brute force: the smallest key and its smallest index, and the second smallest key of the multiset"""
    tgt = np.asarray(target, np.float32)[:, :3]
    q = np.asarray(q, np.float32).reshape(-1, 3)
    j, k1, k2 = np.empty(len(q), np.int64), np.empty(len(q), np.float32), np.full(len(q), np.inf, np.float32)
    for a in range(0, len(q), chunk):
        K = keys_f32(q[a:a + chunk], tgt)
        r = np.arange(len(K))
        ja = K.argmin(axis=1)                      # the first occurrence of the minimum: the smaller index
        j[a:a + chunk], k1[a:a + chunk] = ja, K[r, ja]
        if len(tgt) > 1:
            K[r, ja] = np.inf
            k2[a:a + chunk] = K.min(axis=1)
    return j, k1, k2


def root_f32(x):
    """float64(float32(sqrt(float64(x)))): the correctly rounded fp32 square root, widened"""
    return np.sqrt(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)


def skip_test(q, anchor, key1, key2):
    """bool per point: True where max_first < min_second (:47-51)"""
    dx, dy, dz = (q[:, a] - anchor[:, a] for a in range(3))
    d = root_f32((dx * dx + dy * dy) + dz * dz)
    with np.errstate(invalid="ignore"):
        return root_f32(key1) + d < root_f32(key2) - d


class GICPST(gr.GICP):
    """the vectorised statement; set_target / set_source (gicp_reference.GICP's) and reset() drop the anchors"""

    def __init__(self, d_max=FLT_MAX):
        super().__init__(d_max)
        self.state = None       # dict(corr int64, key1, key2 float32, anchor (ns, 3) float32, M (ns, 3, 3), searched bool)
        self.series, self.poses = [], []

    def set_target(self, pts, cov):
        super().set_target(pts, cov)
        self.state = None

    def set_source(self, pts, cov):
        super().set_source(pts, cov)
        self.state = None

    def reset(self):
        self.state = None

    def update(self, T):
        """update_correspondences (:25-77)"""
        T = np.asarray(T, np.float64)
        ns = len(self.source)
        q = nn.transform_f32(self.source, T.astype(np.float32))
        if self.state is None:
            self.state = dict(corr=np.full(ns, -1, np.int64), key1=np.zeros(ns, np.float32), key2=np.zeros(ns, np.float32),
                              anchor=np.zeros((ns, 3), np.float32), M=np.zeros((ns, 3, 3)), searched=np.ones(ns, bool))
            skip = np.zeros(ns, bool)
        else:
            skip = skip_test(q, self.state["anchor"], self.state["key1"], self.state["key2"])
        st = self.state
        i = np.flatnonzero(~skip)
        st["searched"] = ~skip
        if len(i):
            j, k1, k2 = two_nearest(self.target, q[i])
            keep = k1.astype(np.float64) < self.d_max * self.d_max
            st["corr"][i], st["key1"][i], st["key2"][i], st["anchor"][i] = np.where(keep, j, -1), k1, k2, q[i]
            ik, R = i[keep], T[:3, :3]
            if len(ik):
                st["M"][ik] = np.linalg.inv(self.cov_t[j[keep]] + R @ self.cov_s[ik] @ R.T)
        self.corr = (st["corr"], st["key1"], st["M"][st["corr"] >= 0])

    def sums(self, T, descending=False):
        """cost, H, b of the state as it is at T (:87-119), summed first to last or last to first"""
        c, H, b = self._terms(np.asarray(T, np.float64))
        return float(gr.ordered_sum(c, descending)), gr.ordered_sum(H, descending), gr.ordered_sum(b, descending)

    def linearize(self, T):
        self.update(T)
        self.series.append(self.num_searched())
        self.poses.append(np.array(T, np.float64))
        return self.sums(T)

    def num_searched(self):
        return int(self.state["searched"].sum())

    def align(self, guess, **kw):
        """computeTransformation (:19-22): the anchors dropped, then gicp_reference.GICP.align; series / poses: the number searched and the pose of
        every linearisation of this solve"""
        self.reset()
        self.series, self.poses = [], []
        return super().align(guess, **kw)


class Literal:
    """fast_gicp_st_impl.hpp:25-120 point by point, with the reference's 4x4 matrices (covariances padded with a zero row and column, RCR(3,3) = 1, the
    full 4x4 inverse, M(3,3) = 0, 4-vectors with w = 1, the 4x6 Jacobian) and scalar fp32 arithmetic for the query, the keys and the skip test"""

    def __init__(self, source, cov_s, target, cov_t, d_max=FLT_MAX):
        self.src, self.tgt = np.asarray(source, np.float32)[:, :3], np.asarray(target, np.float32)[:, :3]
        self.cov_s, self.cov_t, self.d_max = np.asarray(cov_s, np.float64), np.asarray(cov_t, np.float64), float(d_max)
        self.anchors = []
        n = len(self.src)
        self.corr, self.sq, self.sq2, self.M, self.searched = [-1] * n, [np.float32(0)] * n, [np.float32(0)] * n, [np.zeros((4, 4)) for _ in range(n)], [False] * n

    @staticmethod
    def _key(a, b):
        d = a - b                                                     # float32 arrays: each operation below rounds to fp32
        return np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])

    def update(self, T):
        T = np.asarray(T, np.float64)
        trans = T.astype(np.float32)
        first = not self.anchors
        if first:
            self.anchors = [None] * len(self.src)
        for i, p in enumerate(self.src):
            pt = np.array([np.float32(np.float32(np.float32(trans[r, 0] * p[0] + trans[r, 1] * p[1]) + trans[r, 2] * p[2]) + trans[r, 3]) for r in range(3)], np.float32)
            self.searched[i] = True
            if not first:
                d = float(np.float32(np.sqrt(np.float64(self._key(pt, self.anchors[i])))))
                max_first = float(np.float32(np.sqrt(np.float64(self.sq[i])))) + d
                min_second = float(np.float32(np.sqrt(np.float64(self.sq2[i])))) - d
                if max_first < min_second:
                    self.searched[i] = False
                    continue
            ranked = sorted((self._key(pt, b), j) for j, b in enumerate(self.tgt))[:2]
            self.corr[i] = ranked[0][1] if float(ranked[0][0]) < self.d_max * self.d_max else -1
            self.sq[i] = ranked[0][0]
            self.sq2[i] = ranked[1][0] if len(ranked) > 1 else np.float32(np.inf)
            self.anchors[i] = pt
            if self.corr[i] < 0:
                continue
            cA, cB = np.zeros((4, 4)), np.zeros((4, 4))
            cA[:3, :3], cB[:3, :3] = self.cov_s[i], self.cov_t[self.corr[i]]
            RCR = cB + T @ cA @ T.T
            RCR[3, 3] = 1.0
            self.M[i] = np.linalg.inv(RCR)
            self.M[i][3, 3] = 0.0

    def linearize(self, T, want_H=True):
        T = np.asarray(T, np.float64)
        if want_H:
            self.update(T)
        cost, H, b = 0.0, np.zeros((6, 6)), np.zeros(6)
        for i in range(len(self.src)):
            j = self.corr[i]
            if j < 0:
                continue
            a = T @ np.append(self.src[i].astype(np.float64), 1.0)
            e = np.append(self.tgt[j].astype(np.float64), 1.0) - a
            cost += float(e @ self.M[i] @ e)
            if not want_H:
                continue
            J = np.zeros((4, 6))
            J[:3, :3] = skew(a[:3])
            J[:3, 3:] = -np.eye(3)
            H += J.T @ self.M[i] @ J
            b += J.T @ self.M[i] @ e
        return cost, H, b

    def compute_error(self, T):
        return self.linearize(T, want_H=False)[0]
