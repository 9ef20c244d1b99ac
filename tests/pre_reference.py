"""An independent reference for the stages either side of the registration operator: B3 the pcl::VoxelGrid leaf filter, B2 de-skew and B9
re-framing.  numpy only; nothing here is taken from the product or from oracle/ -- each function is written from the definition of the
operation (PCL's voxel_grid.hpp for the filter, src/RGC_odometer.cpp:1441-1481 and :1495-1514 for the other two), so that the oracle and
the GPU can both be held to it.

Leaf filter (bit-exact by construction: fp32 multiply, floor, add and divide are correctly rounded everywhere):
    inv = fp32(1) / fp32(leaf);  ijk = floor(fp32(p * inv));  min_b / max_b = floor(fp32(min_p * inv)) / floor(fp32(max_p * inv));
    div = max_b - min_b + 1;  dx dy dz > INT_MAX -> the input, unfiltered;  idx = i + j dx + k dx dy (int64);
    one output per occupied leaf in ascending idx = fp32 running sum of x, y, z, intensity in ASCENDING POINT INDEX / fp32(count).
De-skew and re-framing: np.longdouble (64-bit mantissa on x86), from the definition of slerp (Shoemake's sine weights) and of the rotation
matrix of a quaternion; only `s` is fp32, as the reference's expression types make it."""
import numpy as np

INT_MAX = 2147483647
LD = np.longdouble


class LeafFilterResult:
    """out (m, 4) float32; leaf_index (m,) int64 (None when unfiltered); members(j) -> point indices of output j in summation order;
    minb, div (3,) int64; unfiltered: the leaf grid has more than INT_MAX leaves, out is the input."""

    def __init__(self, out, leaf_index, order, start, minb, div, unfiltered):
        self.out, self.leaf_index, self.order, self.start, self.minb, self.div, self.unfiltered = out, leaf_index, order, start, minb, div, unfiltered

    def members(self, j):
        return self.order[self.start[j]:self.start[j + 1]]

    @property
    def fullest(self):
        return int(np.diff(self.start).max()) if self.start is not None else 0


def four_columns(xyzi):
    """(n, >= 3) -> (n, 4) float32: x, y, z and the intensity column, 0 where the input has none (a 12-byte point)"""
    p = np.asarray(xyzi, dtype=np.float32)
    out = np.zeros((p.shape[0], 4), np.float32)
    c = min(4, p.shape[1])
    out[:, :c] = p[:, :c]
    return out


def leaf_coords(xyz, leaf):
    """floor(fp32(p * inv)) per coordinate, as int64"""
    inv = np.float32(1) / np.float32(leaf)
    prod = np.asarray(xyz, np.float32) * inv           # fp32 * fp32 -> fp32
    assert prod.dtype == np.float32
    return np.floor(prod).astype(np.int64)


def voxelgrid(xyzi, leaf):
    p = four_columns(xyzi)
    n = p.shape[0]
    if n == 0:
        return LeafFilterResult(p, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(3, np.int64), np.zeros(3, np.int64), False)
    assert np.isfinite(p[:, :3]).all(), "the reference filters finite clouds only"
    ijk = leaf_coords(p[:, :3], leaf)
    # PCL: min_b = floor(min_p * inv), max_b = floor(max_p * inv) from getMinMax3D's fp32 extremes
    minb = leaf_coords(p[:, :3].min(axis=0)[None, :], leaf)[0]
    maxb = leaf_coords(p[:, :3].max(axis=0)[None, :], leaf)[0]
    div = maxb - minb + 1
    if int(div[0]) * int(div[1]) * int(div[2]) > INT_MAX:     # python ints: no overflow
        return LeafFilterResult(p.copy(), None, None, None, minb, div, True)
    c = ijk - minb
    assert (c >= 0).all() and (c < div).all()
    idx = c[:, 0] + c[:, 1] * div[0] + c[:, 2] * div[0] * div[1]
    order = np.lexsort((np.arange(n), idx))                   # by leaf, then by point index
    sidx = idx[order]
    head = np.ones(n, bool)
    head[1:] = sidx[1:] != sidx[:-1]
    start = np.flatnonzero(head)
    m = len(start)
    count = np.diff(np.append(start, n))
    sums = np.zeros((m, 4), np.float32)
    live = np.arange(m)
    for r in range(int(count.max())):                         # the r-th member of every leaf that has one: a sequential fp32 sum per leaf
        live = live[count[live] > r]
        sums[live] += p[order[start[live] + r]]
    assert sums.dtype == np.float32
    out = sums / count.astype(np.float32)[:, None]
    assert out.dtype == np.float32
    return LeafFilterResult(out, sidx[start], order, np.append(start, n).astype(np.int64), minb, div, False)


def explain_mismatch(ref, got):
    """which output differs first, and whether it is the count, the membership / order (the sum of the members in another order fits) or the sum"""
    if got.shape != ref.out.shape:
        return "shape %s, reference %s" % (got.shape, ref.out.shape)
    bad = np.flatnonzero((got.view(np.uint32) != ref.out.view(np.uint32)).any(axis=1))
    if len(bad) == 0:
        return "equal"
    j = int(bad[0])
    txt = "%d of %d outputs differ; first: output %d got %s reference %s" % (len(bad), len(got), j, got[j], ref.out[j])
    if ref.leaf_index is not None:
        mem = ref.members(j)
        txt += " leaf index %d, %d members (points %s...)" % (ref.leaf_index[j], len(mem), mem[:6])
    return txt


# ---- de-skew and re-framing ------------------------------------------------------------------------------------------------------
def deskew_s(intensity):
    """s = 1 - (intensity - int(intensity)) / SCAN_PERIOD with SCAN_PERIOD = 0.1f: float - int -> float, float / float -> float, int - float -> float
    (src/RGC_odometer.cpp:1448 and the like); the `double s =` then widens the fp32 value"""
    i = np.asarray(intensity, np.float32)
    frac = i - np.trunc(i).astype(np.int32).astype(np.float32)
    s = np.float32(1) - frac / np.float32(0.1)
    assert s.dtype == np.float32
    return s


def rotation_matrix(q_xyzw):
    """R(q) of the textbook unit-quaternion formula, (..., 3, 3) longdouble.  Applied as it stands to a quaternion slightly off unit norm, which is what
    the reference's Eigen `q * v` evaluates (algebraically), not q v q^-1."""
    q = np.asarray(q_xyzw, LD)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3), LD)
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - z * w); R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w); R[..., 2, 1] = 2 * (y * z + x * w); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def quat_inverse(q_xyzw):
    """conjugate over squared norm (Eigen's Quaternion::inverse, RGC_odometer.cpp:1444), longdouble"""
    q = np.asarray(q_xyzw, np.float64).astype(LD)
    n2 = (q * q).sum()
    return np.array([-q[0], -q[1], -q[2], q[3]], LD) / n2


def slerp_from_identity(s, q1_xyzw):
    """slerp(s; identity, q1), (len(s), 4) longdouble: Shoemake's weights sin((1 - s) th) / sin th and sin(s th) / sin th with cos th = |<identity, q1>|,
    the shorter arc (q1 negated when the dot product is negative); their limit 1 - s and s when th is 0."""
    s = np.asarray(s).astype(LD)
    q1 = np.asarray(q1_xyzw, LD)
    d = q1[3]
    if d < 0:
        q1, d = -q1, -d
    if d >= 1:
        w0, w1 = 1 - s, s
    else:
        th = np.arccos(d)
        w0, w1 = np.sin((1 - s) * th) / np.sin(th), np.sin(s * th) / np.sin(th)
    out = w1[:, None] * q1[None, :]
    out[:, 3] += w0
    return out


def deskew(xyzi, q_last_curr_xyzw, t_last_curr):
    """p' = R(slerp(s; identity, q^-1)) (p - s t), (n, 3) longdouble"""
    p = np.asarray(xyzi, np.float32)
    s = deskew_s(p[:, 3])
    qs = slerp_from_identity(s, quat_inverse(q_last_curr_xyzw))
    v = p[:, :3].astype(LD) - s.astype(LD)[:, None] * np.asarray(t_last_curr, np.float64).astype(LD)[None, :]
    return np.einsum("nij,nj->ni", rotation_matrix(qs), v)


def transform(xyz, q_xyzw, t):
    """R(q) p + t, (n, 3) longdouble"""
    p = np.asarray(xyz, np.float32)[:, :3].astype(LD)
    R = rotation_matrix(np.asarray(q_xyzw, np.float64).astype(LD))
    return p @ R.T + np.asarray(t, np.float64).astype(LD)[None, :]


def ulp_bound(ref, p_abs, t_abs):
    """the tolerance of a stored fp32 coordinate against the high-precision value `ref`: one fp32 ulp at the reference's value, plus the fp64 error of the
    terms it is summed from where the result cancels, 8 * 2^-53 * (|p| + |t|)"""
    ulp = np.spacing(np.abs(np.asarray(ref, np.float64)).astype(np.float32)).astype(np.float64)
    return ulp + 8.0 * 2.0 ** -53 * (np.asarray(p_abs, np.float64) + np.asarray(t_abs, np.float64))[:, None]


def worst_in_ulps(got, ref):
    """(largest |got - ref| in fp32 ulps at the reference's value, its flat position)"""
    ref64 = np.asarray(ref, np.float64)
    ulp = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    e = np.abs(np.asarray(got, np.float64) - np.asarray(ref, LD)).astype(np.float64) / ulp
    k = int(np.argmax(e))
    return float(e.flat[k]), k
