"""NDT registration (P2D / D2D) on a Gaussian voxel map, restated in numpy fp64 -- the reference of tests/test_ndt_reference.py and tests/test_gpu_ndt.py.
Written from the formulas of fast_gicp::NDTCuda (src/fast_gicp/cuda/ndt_cuda.cu, ndt_compute_derivatives.cu, gaussian_voxelmap.cu,
covariance_regularization.cu, find_voxel_correspondences.cu of the reference, which is fp32 CUDA) and shares no code with the product: numpy `eigh` and
`inv`, a table of voxels keyed by coordinate, LsqRegistration's LM driver (lsq_registration_impl.hpp:53-79,125-172) in plain Python.

Arithmetic: input points fp32, widened to fp64 before anything else.  The per-voxel sums run SEQUENTIALLY over the voxel's points in ascending (or,
for the order-to-order spread the GPU test measures, descending) point index; numpy's cumulative sum is that loop."""
import numpy as np

P2D, D2D = 0, 1
DIRECT27, DIRECT7, DIRECT1, DIRECT_RADIUS = 0, 1, 2, 3
MIN_EIG_FLOOR = 1e-3


def offsets(method, radius=0.0):
    """the voxel offsets of a neighbour method, in the reference's order (ndt_cuda.cu:35-88)"""
    if method == DIRECT1:
        return np.zeros((1, 3), np.int64)
    if method == DIRECT7:
        return np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.int64)
    if method == DIRECT27:
        return np.array([[i - 1, j - 1, k - 1] for i in range(3) for j in range(3) for k in range(3)], np.int64)
    rng = int(np.ceil(radius))
    out = []
    for i in range(-rng, rng + 1):
        for j in range(-rng, rng + 1):
            for k in range(-rng, rng + 1):
                if np.sqrt(float(i * i + j * j + k * k)) <= radius + 1e-3:
                    out.append([i, j, k])
    return np.array(out, np.int64).reshape(-1, 3)


def voxel_coord(x, res):
    """floor(x / res - 0.5) per axis (vector3_hash.cuh:35-37), x fp64"""
    return np.floor(np.asarray(x, np.float64) / res - 0.5).astype(np.int64)


def wall_distance(x, res):
    """distance of every coordinate to the nearest voxel wall, in units of res"""
    u = np.asarray(x, np.float64) / res - 0.5
    return np.abs(u - np.round(u))


def min_eig(cov):
    """MIN_EIG (covariance_regularization.cu:83-100): eigenvalues raised to at least 1e-3, recomposed"""
    w, V = np.linalg.eigh(0.5 * (cov + cov.T))
    return (V * np.maximum(w, MIN_EIG_FLOOR)) @ V.T


_KEY = 1 << 20


def _keys(c):
    c = np.asarray(c, np.int64) + _KEY
    return (c[..., 0] << 42) | (c[..., 1] << 21) | c[..., 2]


class VoxelMap:
    """coords (V, 3) int64 sorted by key, n (V,), mean (V, 3), cov_raw / cov (V, 3, 3) before / after MIN_EIG (gaussian_voxelmap.cu:122-231)"""

    def __init__(self, points, res, descending=False):
        p = np.asarray(points, np.float32)[:, :3].astype(np.float64)
        c = voxel_coord(p, res)
        assert np.abs(c).max() < _KEY
        k = _keys(c)
        order = np.argsort(k, kind="stable")                 # ascending point index inside a voxel
        ks = k[order]
        first = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
        last = np.r_[first[1:], len(ks)]
        V = len(first)
        self.res, self.keys, self.coords = float(res), ks[first], c[order[first]]
        self.n = (last - first).astype(np.int64)
        self.mean, self.cov_raw, self.cov = np.zeros((V, 3)), np.zeros((V, 3, 3)), np.zeros((V, 3, 3))
        iu = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        for v in range(V):
            q = p[order[first[v]:last[v]]]
            if descending:
                q = q[::-1]
            n = float(len(q))
            s1 = np.cumsum(q, axis=0)[-1]                                               # sequential, in the order of q
            s2 = np.cumsum(np.stack([q[:, a] * q[:, b] for a, b in iu], axis=1), axis=0)[-1]
            m = s1 / n
            C = np.zeros((3, 3))
            for t, (a, b) in enumerate(iu):                                             # cov = (sum p p^T - mean (sum p)^T) / n
                C[a, b] = C[b, a] = (s2[t] - m[a] * s1[b]) / n
            self.mean[v], self.cov_raw[v], self.cov[v] = m, C, min_eig(C)

    def lookup(self, coords):
        """voxel index of every coordinate row, -1 where there is none"""
        k = _keys(coords)
        i = np.clip(np.searchsorted(self.keys, k), 0, len(self.keys) - 1)
        return np.where(self.keys[i] == k, i, -1)

    def as_dict(self):
        return {tuple(int(x) for x in self.coords[v]): v for v in range(len(self.n))}


def skew(q):
    S = np.zeros(q.shape[:-1] + (3, 3))
    S[..., 0, 1], S[..., 0, 2] = -q[..., 2], q[..., 1]
    S[..., 1, 0], S[..., 1, 2] = q[..., 2], -q[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -q[..., 1], q[..., 0]
    return S


def so3_exp(w):
    """so3_exp (so3.hpp:58-77) -> rotation matrix"""
    w = np.asarray(w, np.float64)
    th2 = float(w @ w)
    if th2 < 1e-10:
        imag, real = 0.5 - th2 / 48.0 + th2 * th2 / 3840.0, 1.0 - th2 / 8.0 + th2 * th2 / 384.0
    else:
        th = np.sqrt(th2)
        imag, real = np.sin(0.5 * th) / th, np.cos(0.5 * th)
    qw, (qx, qy, qz) = real, imag * w
    return np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                     [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                     [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])


def increment(d, x0):
    """the driver's update (lsq_registration_impl.hpp:139-143): xi = [so3_exp(d[:3]) | d[3:]] * x0"""
    delta = np.eye(4)
    delta[:3, :3], delta[:3, 3] = so3_exp(d[:3]), d[3:]
    return delta @ x0, delta


class NDT:
    def __init__(self, resolution=1.0, mode=D2D, method=DIRECT7, radius=0.0):
        self.res, self.mode, self.offs = float(resolution), mode, offsets(method, radius)
        self.target = self.source = None
        self.tmap = self.smap = None
        self.corr = None

    def set_target(self, pts):
        self.target, self.tmap, self.corr = np.asarray(pts, np.float32)[:, :3], None, None

    def set_source(self, pts):
        self.source, self.smap, self.corr = np.asarray(pts, np.float32)[:, :3], None, None

    def build(self):
        if self.tmap is None:
            self.tmap = VoxelMap(self.target, self.res)
        if self.mode == D2D and self.smap is None:
            self.smap = VoxelMap(self.source, self.res)

    def elements(self):
        if self.mode == D2D:
            return self.smap.mean, self.smap.cov
        return self.source.astype(np.float64), None

    def transformed(self, T):
        a, _ = self.elements()
        return a @ T[:3, :3].T + T[:3, 3]

    def _terms(self, T, frozen_w=None):
        """cost, H, b and the per-term pieces over the frozen (element, voxel) list"""
        e_idx, v_idx, R_lin = self.corr
        a, covA = self.elements()
        R, t = T[:3, :3], T[:3, 3]
        q = a[e_idx] @ R.T + t
        e = self.tmap.mean[v_idx] - q
        if self.mode == D2D:
            M = np.linalg.inv(self.tmap.cov[v_idx] + R_lin @ covA[e_idx] @ R_lin.T)
        else:
            M = np.linalg.inv(self.tmap.cov[v_idx])
        r2 = self.res * self.res
        w = r2 / (r2 + np.einsum("ni,ni->n", e, e)) if frozen_w is None else frozen_w
        J = np.concatenate([skew(q), -np.broadcast_to(np.eye(3), (len(q), 3, 3))], axis=2)
        Me = np.einsum("nij,nj->ni", M, e)
        cost = float(np.sum(w * np.einsum("ni,ni->n", e, Me)))
        H = np.einsum("n,nia,nij,njb->ab", w, J, M, J)
        b = np.einsum("n,nia,ni->a", w, J, Me)
        return cost, H, b, w

    def linearize(self, T):
        """update_correspondences + compute_error(H, b) (ndt_cuda_impl.hpp:81-85): returns cost, H, b"""
        T = np.asarray(T, np.float64)
        self.build()
        c = voxel_coord(self.transformed(T), self.res)
        e_idx, v_idx = [], []
        for o in self.offs:                                   # every (element, offset) hit is a term of its own
            v = self.tmap.lookup(c + o)
            ok = v >= 0
            ok[ok] = self.tmap.n[v[ok]] > 6                   # num_points <= 6: skipped (ndt_compute_derivatives.cu:61-63)
            e_idx.append(np.flatnonzero(ok))
            v_idx.append(v[ok])
        self.corr = (np.concatenate(e_idx), np.concatenate(v_idx), T[:3, :3].copy())
        cost, H, b, _ = self._terms(T)
        return cost, H, b

    def num_terms(self):
        return len(self.corr[0])

    def compute_error(self, T, frozen_w=None):
        return self._terms(np.asarray(T, np.float64), frozen_w)[0]

    def weights(self, T):
        return self._terms(np.asarray(T, np.float64))[3]

    def align(self, guess, max_iterations=25, lm_max_iterations=10, rotation_eps=2e-3, translation_eps=1e-6, init_lambda_factor=1e-9):
        """LsqRegistration::computeTransformation (lsq_registration_impl.hpp:53-79) with step_lm (:125-172): returns T (fp64), iterations, converged,
        lm_failed, final Hessian"""
        def is_converged(delta):
            m = max(np.abs(delta[:3, :3] - np.eye(3)).max() / rotation_eps, np.abs(delta[:3, 3]).max() / translation_eps)
            return m < 1
        x0 = np.asarray(guess, np.float32).astype(np.float64).copy()
        x0[3] = [0, 0, 0, 1]
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


def scene(rng, n, center=(100.0, -60.0, 2.0), half=12.0, noise=0.02):
    """a box room with a floor and a few inner walls around `center`: planar patches dense enough for voxels of more than 6 points, at coordinates of
    about 100 m (what makes sum p p^T - mean (sum p)^T cancel).  (n, 3) float32."""
    c = np.asarray(center, np.float64)
    kinds = rng.integers(0, 6, n)
    u, v = rng.uniform(-half, half, n), rng.uniform(-half, half, n)
    h = rng.uniform(0.0, 3.0, n)
    p = np.zeros((n, 3))
    f = kinds <= 1
    p[f] = np.stack([u[f], v[f], np.zeros(f.sum())], 1)                              # floor
    for k, (axis, pos) in zip((2, 3, 4, 5), ((0, -half), (0, half * 0.6), (1, -half * 0.7), (1, half))):
        m = kinds == k
        q = np.stack([u[m], v[m], h[m]], 1)
        q[:, axis] = pos
        p[m] = q
    p += rng.normal(0.0, noise, p.shape)
    return (p + c).astype(np.float32)


def random_pose(rng, max_t=0.3, max_deg=3.0, about=(0.0, 0.0, 0.0)):
    """a random SE(3) within max_t metres / max_deg degrees, rotating about the point `about`"""
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    R = so3_exp(ax * np.deg2rad(rng.uniform(0.3, 1.0) * max_deg))
    t = rng.normal(size=3)
    t *= rng.uniform(0.3, 1.0) * max_t / np.linalg.norm(t)
    T = np.eye(4)
    a = np.asarray(about, np.float64)
    T[:3, :3], T[:3, 3] = R, a - R @ a + t
    return T


def off_the_walls(rng, pts, poses, res_list, make, tol=1e-4, noffs=None):
    """Regenerates (with `make(k)` -> k new points) every point of pts that, under one of `poses`, lies within tol * res of a voxel wall for one of
    res_list.  Returns the points and the share of points that had to be regenerated."""
    pts = np.array(pts, np.float32)
    redone = np.zeros(len(pts), bool)
    for _ in range(20):
        bad = np.zeros(len(pts), bool)
        p = pts.astype(np.float64)
        for T in poses:
            q = p @ T[:3, :3].T + T[:3, 3]
            for res in res_list:
                bad |= (wall_distance(q, res) < tol).any(axis=1)
        if not bad.any():
            break
        pts[bad] = make(int(bad.sum()))
        redone |= bad
    assert not bad.any()
    return pts, float(redone.mean())
