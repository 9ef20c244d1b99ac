"""An independent fp64 reference for the voxel stage of FastVGICP: voxel table, correspondences, H / b / cost (numpy only; nothing from
oracle/).

Its input is the points (fp32) and their per-point 3x3 covariances, so a mismatch against it is the voxel or linearisation code's fault and
not the k-NN's (tests/knn_reference.py holds that stage).  Every line follows the cited reference:

  * voxel coordinate: ``floor(x / res - 0.5)`` of the fp32 coordinate widened to fp64, a true division (fast_vgicp_voxel.hpp:158-160);
  * voxel table: ADDITIVE and ADDITIVE_WEIGHTED are both AdditiveGaussianVoxel (sums in cloud order, then / num_points, :105-122);
    MULTIPLICATIVE is the 4x4 with (3,3) = 1, inverted on append and again at finalize (:79-100), written here as the reference writes it;
  * correspondences: the transformed point ``((r0 x + r1 y) + r2 z) + t`` per row in fp64 (numpy ufuncs: nothing is contracted), its
    coordinate plus every offset of DIRECT1 / DIRECT7 / DIRECT27 in the reference's order (:10-44), ``RCR = C_B + R C_A R^T`` and its
    inverse (fast_vgicp_impl.hpp:73-115);
  * cost, H and b with ``w = sqrt(num_points)`` (:119-180); compute_error over the correspondences frozen by the last linearisation
    (:183-205).

Voxel tables come out in cell order, x fastest (``cell_order``).  ``wall_values`` / ``wall_sources`` build points on voxel walls and a few
ulps either side of them, and say how many of them a subtly different computation (``x * (1 / res)``, another summation order of the pose
product) would put into another cell.
"""
from __future__ import annotations

import numpy as np

OFFSETS = {
    "DIRECT1": np.array([[0, 0, 0]]),
    "DIRECT7": np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]),
    "DIRECT27": np.array([[i - 1, j - 1, k - 1] for i in range(3) for j in range(3) for k in range(3)]),
}
METHODS = ("DIRECT27", "DIRECT7", "DIRECT1")              # NeighborSearchMethod's enum order (gicp_settings.hpp:8)
MODES = ("ADDITIVE", "ADDITIVE_WEIGHTED", "MULTIPLICATIVE")  # VoxelAccumulationMode's enum order (gicp_settings.hpp:10)

_BIAS, _SPAN = 1 << 20, 1 << 21                            # packed keys: |coordinate| < 2^20 cells


def voxel_coords(P, res: float) -> np.ndarray:
    """(n, 3) int64: floor(x / res - 0.5) per axis, x the fp32 coordinate in fp64"""
    X = np.asarray(P, np.float32)[:, :3].astype(np.float64)
    return np.floor(X / float(res) - 0.5).astype(np.int64)


def _key(c) -> np.ndarray:
    c = np.asarray(c, np.int64) + _BIAS
    assert c.min(initial=0) >= 0 and c.max(initial=0) < _SPAN, "voxel coordinate out of the packed range"
    return (c[..., 2] * _SPAN + c[..., 1]) * _SPAN + c[..., 0]          # ascending key = cell order, x fastest


def cell_order(coords) -> np.ndarray:
    """the permutation that puts voxel coordinates (m, 3) into cell order, x fastest"""
    c = np.asarray(coords)
    return np.lexsort((c[:, 0], c[:, 1], c[:, 2]))


def in_cell_order(table: dict) -> dict:
    o = cell_order(table["coords"])
    return {k: np.asarray(v)[o] for k, v in table.items()}


def _inv4_block(C3):
    """inverse of the 4x4 [[C, 0], [0, 1]] written out as the reference does (Matrix4d::inverse), for (m, 3, 3) C"""
    A = np.zeros(C3.shape[:-2] + (4, 4))
    A[..., :3, :3] = C3
    A[..., 3, 3] = 1.0
    return np.linalg.inv(A)


def voxel_table(P, cov, res: float, mode: str = "ADDITIVE") -> dict:
    """Gaussian voxel map of points P (n, >=3, fp32) with per-point covariances cov (n, 3, 3): dict(coords (m, 3) int64, num (m,) int64,
    mean (m, 3), cov (m, 3, 3)) in cell order, x fastest"""
    X = np.asarray(P, np.float32)[:, :3].astype(np.float64)
    cov = np.asarray(cov, np.float64).reshape(-1, 3, 3)
    keys = _key(voxel_coords(P, res))
    uk, inv, num = np.unique(keys, return_inverse=True, return_counts=True)
    m = len(uk)
    if mode in ("ADDITIVE", "ADDITIVE_WEIGHTED"):
        msum, csum = np.zeros((m, 3)), np.zeros((m, 3, 3))
        np.add.at(msum, inv, X)                                          # cloud order, one point at a time
        np.add.at(csum, inv, cov)
        mean, vcov = msum / num[:, None], csum / num[:, None, None]
    elif mode == "MULTIPLICATIVE":
        Ci = _inv4_block(cov)                                            # (n, 4, 4): C^-1 in the 3x3 block, 1 at (3, 3)
        X4 = np.concatenate([X, np.ones((len(X), 1))], axis=1)
        csum, msum = np.zeros((m, 4, 4)), np.zeros((m, 4))
        np.add.at(csum, inv, Ci)
        np.add.at(msum, inv, np.einsum("nij,nj->ni", Ci, X4))
        csum[:, 3, 3] = 1.0                                              # finalize: cov(3, 3) = 1, mean[3] = 1
        msum[:, 3] = 1.0
        C = np.linalg.inv(csum)
        mean, vcov = np.einsum("mij,mj->mi", C, msum)[:, :3], C[:, :3, :3]
    else:
        raise ValueError(mode)
    c = np.stack([uk % _SPAN, (uk // _SPAN) % _SPAN, uk // (_SPAN * _SPAN)], axis=1) - _BIAS
    return dict(coords=c, num=num.astype(np.int64), mean=mean, cov=vcov)


def transform(T, P) -> np.ndarray:
    """((r0 x + r1 y) + r2 z) + t per row, fp64, no fused multiply-add"""
    T = np.asarray(T, np.float64)
    X = np.asarray(P, np.float32)[:, :3].astype(np.float64)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)


def correspondences(src, src_cov, table: dict, T, res: float, method: str) -> dict:
    """update_correspondences (fast_vgicp_impl.hpp:73-115): (source index, voxel index) pairs in (source, offset) order and the
    frozen Mahalanobis matrices M = (C_B + R C_A R^T)^-1"""
    q = transform(T, src)
    c = np.floor(q / float(res) - 0.5).astype(np.int64)
    off = OFFSETS[method]
    cand = _key(c[:, None, :] + off[None, :, :]).reshape(-1)
    vk = _key(table["coords"])
    o = np.argsort(vk)
    pos = np.clip(np.searchsorted(vk[o], cand), 0, len(vk) - 1)
    hit = vk[o][pos] == cand
    si = np.repeat(np.arange(len(q)), len(off))[hit]
    vi = o[pos[hit]]
    R = np.asarray(T, np.float64)[:3, :3]
    CA = np.asarray(src_cov, np.float64).reshape(-1, 3, 3)[si]
    RCR = table["cov"][vi] + np.einsum("ij,njk,lk->nil", R, CA, R)
    # RCR(3, 3) = 1, inverse, (3, 3) = 0: the 3x3 block of the 4x4's inverse
    M = _inv4_block(RCR)[:, :3, :3]
    return dict(src=si, vox=vi, M=M, T=np.asarray(T, np.float64).copy())


def _cost_terms(src, table, corr, T):
    q = transform(T, src)[corr["src"]]
    e = table["mean"][corr["vox"]] - q
    w = np.sqrt(table["num"][corr["vox"]].astype(np.float64))
    Me = np.einsum("nij,nj->ni", corr["M"], e)
    return q, e, w, Me


def linearize(src, src_cov, table: dict, T, res: float, method: str):
    """FastVGICP::linearize (fast_vgicp_impl.hpp:119-180): (cost, H (6, 6), b (6,), correspondences)"""
    corr = correspondences(src, src_cov, table, T, res, method)
    q, e, w, Me = _cost_terms(src, table, corr, T)
    cost = float(np.sum(w * np.einsum("ni,ni->n", e, Me)))
    J = np.zeros((len(q), 3, 6))
    J[:, 0, 1], J[:, 0, 2] = -q[:, 2], q[:, 1]                          # skewd(q) | -I
    J[:, 1, 0], J[:, 1, 2] = q[:, 2], -q[:, 0]
    J[:, 2, 0], J[:, 2, 1] = -q[:, 1], q[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = -1.0
    H = np.einsum("n,nai,nab,nbj->ij", w, J, corr["M"], J)
    b = np.einsum("n,nai,na->i", w, J, Me)
    return cost, H, b, corr


def compute_error(src, table: dict, corr: dict, T) -> float:
    """FastVGICP::compute_error (fast_vgicp_impl.hpp:183-205) over the correspondences of the last linearisation"""
    _, e, w, Me = _cost_terms(src, table, corr, T)
    return float(np.sum(w * np.einsum("ni,ni->n", e, Me)))


def rel(a, b) -> float:
    """max |a - b| / max |b| (0 where both are 0)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    num, den = float(np.abs(a - b).max(initial=0.0)), float(np.abs(b).max(initial=0.0))
    return 0.0 if num == 0.0 else (num / den if den > 0 else np.inf)


# ---- points on voxel walls ----------------------------------------------------------------------------------------------------------

def _ulps(x: np.ndarray, k: int) -> np.ndarray:
    x = np.asarray(x, np.float32)
    to = np.where(k > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, to)
    return x


def wall_values(res: float, cells, ulps=(-3, -2, -1, 0, 1, 2, 3)) -> np.ndarray:
    """fp32 coordinates at the wall (c + 0.5) * res between cells c - 1 and c and at +-1..3 ulps of it, for every c in cells"""
    w = ((np.asarray(cells, np.float64) + 0.5) * float(res)).astype(np.float32)
    return np.concatenate([_ulps(w, k) for k in ulps])


def floor_mul(x, res: float) -> np.ndarray:
    """the mutant voxel coordinate floor(x * (1 / res) - 0.5)"""
    return np.floor(np.asarray(x, np.float32).astype(np.float64) * (1.0 / float(res)) - 0.5).astype(np.int64)


def floor_div(x, res: float) -> np.ndarray:
    return np.floor(np.asarray(x, np.float32).astype(np.float64) / float(res) - 0.5).astype(np.int64)


def wall_sharpness(res: float, cells) -> float:
    """share of wall_values(res, cells) whose voxel coordinate changes when x / res is computed as x * (1 / res)"""
    x = wall_values(res, cells)
    return float(np.mean(floor_mul(x, res) != floor_div(x, res)))


def wall_sources(res: float, R, cells, rng) -> tuple:
    """Source points whose transformed position lands exactly on a voxel wall on all three axes, each under a pose of its own.
    For source point j (fp32, drawn near the origin) and rotation R, t_j is chosen so that ((r0 x + r1 y) + r2 z) + t_j is the wall
    (c_j + 0.5) * res in fp64, verified by recomputation.  Returns (points (m, 3) fp32, poses (m, 4, 4), walls (m, 3) int64,
    share): walls[j] is the cell the product's order gives (the division decides on which side of the wall), share the fraction of
    (point, axis) whose cell changes under the other summation order r0 x + (r1 y + (r2 z + t))."""
    R = np.asarray(R, np.float64)
    pts, poses, walls = [], [], []
    cells = np.asarray(cells)
    while len(pts) < len(cells):
        p = rng.uniform(-4.0, 4.0, 3).astype(np.float32)
        c = cells[len(pts)] + np.array([0, 1, -1])
        wall = (c.astype(np.float64) + 0.5) * float(res)
        T = np.eye(4)
        T[:3, :3] = R
        s = transform(T, p[None])[0]                                     # ((r0 x + r1 y) + r2 z), t = 0
        T[:3, 3] = wall - s
        if np.array_equal(transform(T, p[None])[0], wall):
            pts.append(p); poses.append(T); walls.append(np.floor(wall / float(res) - 0.5).astype(np.int64))
    pts, poses, walls = np.array(pts, np.float32), np.array(poses), np.array(walls, np.int64)
    X = pts.astype(np.float64)
    other = np.stack([poses[:, a, 0] * X[:, 0] + (poses[:, a, 1] * X[:, 1] + (poses[:, a, 2] * X[:, 2] + poses[:, a, 3]))
                      for a in range(3)], axis=1)
    share = float(np.mean(np.floor(other / float(res) - 0.5).astype(np.int64) != walls))
    return pts, poses, walls, share
