"""An independent numpy reference of RANSAC plane segmentation (rgc_plane_segment), written from the header block of include/rgc_hip.h alone: the
counter-based sampler in Python integers, the model of a triple in float64 in the header's operation order, the score in float32 with explicit separate
multiplies and adds, PCL's sequential loop (and its replay over batches of counts), and the refinement in longdouble with numpy.linalg.eigh.

Beside the results it returns what the tests need to show that a case is decidable -- how close any `iterations >= k` comparison, any collinearity test and
any axis test came to equality -- and the derived error bound of the refined coefficients."""
import math

import numpy as np

MASK = 2 ** 64 - 1
GOLDEN = 0x9E3779B97F4A7C15
PLANE, PERPENDICULAR = 0, 1
DBL_EPSILON = float(np.finfo(np.float64).eps)


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def sample(seed, t, n):
    """the triple of stream position t: distinct by construction"""
    r = [mix((seed + (3 * t + j + 1) * GOLDEN) & MASK) for j in range(3)]
    i0 = r[0] % n
    i1 = (i0 + 1 + r[1] % (n - 1)) % n
    rest = [i for i in range(n) if i not in (i0, i1)] if n <= 64 else None
    k = r[2] % (n - 2)
    if rest is not None:
        i2 = rest[k]
    else:                                          # the k-th index not in {i0, i1}, without the list
        lo, hi = min(i0, i1), max(i0, i1)
        i2 = k if k < lo else (k + 1 if k + 1 < hi else k + 2)
    return i0, i1, i2


def params(threshold, max_iterations=50, probability=0.99, optimize=1, model=PLANE, axis=(0.0, 0.0, 1.0), eps_angle=0.0, seed=0):
    return dict(threshold=float(threshold), max_iterations=int(max_iterations), probability=float(probability), optimize=int(optimize), model=model,
                axis=tuple(float(v) for v in axis), eps_angle=float(eps_angle), seed=int(seed))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def model_of(cloud, ijk, prm):
    """(valid, float32 (a, b, c, d), diagnostics) of a triple; cloud: (n, >=3) float32"""
    with np.errstate(all="ignore"):
        p0, p1, p2 = (np.asarray(cloud[i, :3], np.float32).astype(np.float64) for i in ijk)
        e1, e2 = p1 - p0, p2 - p0
        c = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
        cc, a1, a2 = _dot(c, c), _dot(e1, e1), _dot(e2, e2)
        bound = 1e-12 * (a1 * a2)
        diag = {"cc": float(cc), "bound": float(bound), "axis_gap": None}
        ok = bool(cc > bound)
        nrm = c / np.sqrt(cc)
        d = -_dot(nrm, p0)
        m = np.array([nrm[0], nrm[1], nrm[2], d]).astype(np.float32)
        ok = ok and bool(np.isfinite(nrm).all() and np.isfinite(d) and np.isfinite(m).all())
        if ok and prm["model"] == PERPENDICULAR:
            ax = np.array(prm["axis"], np.float64)
            ax = ax / np.sqrt(_dot(ax, ax))
            v, ce = abs(_dot(nrm, ax)), math.cos(prm["eps_angle"])
            diag["axis_gap"] = float(abs(v - ce))
            ok = not (v < ce)
    return ok, m, diag


def inliers_of(cloud, m, threshold):
    """the strict fp32 rule: fabsf(((a x + b y) + c z) + d) < (float)threshold, every operation rounded to float32 on its own"""
    x, y, z = (np.ascontiguousarray(cloud[:, k], np.float32) for k in range(3))
    a, b, c, d = (np.float32(v) for v in m)
    with np.errstate(all="ignore"):
        ax = a * x
        by = b * y
        s1 = ax + by
        cz = c * z
        s2 = s1 + cz
        v = s2 + d
        return np.abs(v) < np.float32(threshold), v


def stream_length(prm, samples):
    return len(samples) if samples is not None else 10 * prm["max_iterations"]


def triple_at(cloud, prm, samples, t):
    return tuple(int(v) for v in samples[t]) if samples is not None else sample(prm["seed"], t, len(cloud))


def count_at(cloud, prm, samples, t):
    """(count or -1, float32 model, diagnostics) of stream position t"""
    ok, m, diag = model_of(cloud, triple_at(cloud, prm, samples, t), prm)
    if not ok:
        return -1, m, diag
    return int(inliers_of(cloud, m, prm["threshold"])[0].sum()), m, diag


class Decision:
    """PCL's sequential loop as a state machine fed one count at a time (feed returns True when the loop has stopped)"""

    def __init__(self, n, prm, length):
        self.n, self.prm, self.length = n, prm, length
        self.best, self.k, self.iterations, self.skipped, self.positions, self.best_position = -1, 1.0, 0, 0, 0, -1
        self.counts, self.k_margin = [], math.inf
        self.stopped = length == 0

    def feed(self, count):
        assert not self.stopped
        t = self.positions
        self.counts.append(count)
        self.positions += 1
        if count < 0:
            self.skipped += 1
        else:
            if count > self.best:
                self.best, self.best_position = count, t
                w = self.best / self.n
                q = min(max(1.0 - (w * w) * w, DBL_EPSILON), 1.0 - DBL_EPSILON)
                self.k = math.log(1.0 - self.prm["probability"]) / math.log(q)
            self.iterations += 1
            self.k_margin = min(self.k_margin, abs(self.iterations - self.k) / self.k)     # how close `iterations >= k` came to equality
            if self.iterations >= self.k or self.iterations == self.prm["max_iterations"]:
                self.stopped = True
        if self.positions == self.length:
            self.stopped = True
        return self.stopped

    def result(self):
        return dict(counts=np.array(self.counts, np.int32), iterations=self.iterations, skipped=self.skipped, positions=self.positions, best_position=self.best_position,
                    best_count=self.best, k=self.k, k_margin=self.k_margin)


def decide_sequential(n, prm, length, count_of):
    """the definition: one position at a time, nothing evaluated behind the stop"""
    d = Decision(n, prm, length)
    t = 0
    while not d.stopped:
        d.feed(count_of(t))
        t += 1
    return d.result()


def decide_batched(n, prm, length, count_of, batch):
    """what the library does: the counts of a whole batch first, then the loop replayed over them; what lies behind the stop is ignored"""
    d = Decision(n, prm, length)
    t0, launches = 0, 0
    while not d.stopped:
        b = min(batch, length - t0)
        counts = [count_of(t0 + j) for j in range(b)]
        launches += 1
        for c in counts:
            if d.feed(c):
                break
        t0 += b
    r = d.result()
    r["launches"] = launches
    return r


def refine(cloud, mask, m0):
    """the refinement in longdouble: (coefficients float64 unrounded, bound on a normal component, bound on d, eigenvalues) over the points of mask"""
    p = np.asarray(cloud[mask, :3], np.float32).astype(np.longdouble)
    m = len(p)
    cen = p.sum(axis=0) / m
    dlt = p - cen
    S = (dlt[:, :, None] * dlt[:, None, :]).sum(axis=0) / m
    A = (np.abs(dlt[:, :, None] * dlt[:, None, :])).sum(axis=0) / m            # the sums of absolute terms, normalised like S
    ev, V = np.linalg.eigh(S.astype(np.float64))
    v = V[:, 0].copy()
    if _dot(v, np.asarray(m0[:3], np.float64)) < 0:
        v = -v
    d = -float(_dot(v.astype(np.longdouble), cen))
    gap = float(ev[1] - ev[0])
    # backward error of the fixed-order fp64 sums: m 2^-53 relative to the sum of absolute terms of each entry (Frobenius norm over the entries), through
    # the eigenvector's condition 1 / (lambda_1 - lambda_0), times 8 for the 3x3 Jacobi solver
    err_S = float(np.sqrt((A.astype(np.float64) ** 2).sum())) * m * 2.0 ** -53
    bound_n = 8.0 * err_S / gap if gap > 0 else math.inf
    err_cen = float(np.abs(p).sum(axis=0).max() / m) * m * 2.0 ** -53
    bound_d = bound_n * float(np.sqrt((cen.astype(np.float64) ** 2).sum())) * math.sqrt(3.0) + err_cen * math.sqrt(3.0)
    return np.array([v[0], v[1], v[2], d], np.float64), bound_n, bound_d, ev


def run(cloud, prm, samples=None, batch=None):
    """the whole call: the decision, the RANSAC model, the inliers, the refinement.  batch: None = the sequential definition"""
    cloud = np.ascontiguousarray(cloud, np.float32)
    n = len(cloud)
    length = stream_length(prm, samples)
    seen = {}

    def count_of(t):
        if t not in seen:
            seen[t] = count_at(cloud, prm, samples, t)
        return seen[t][0]

    r = decide_sequential(n, prm, length, count_of) if batch is None else decide_batched(n, prm, length, count_of, batch)
    used = [seen[t][2] for t in range(r["positions"])]
    # how close any collinearity test came to its bound (a factor; exact zeros aside) and any axis test to cos(eps_angle)
    r["collinear_factor"] = min([max(d["cc"] / d["bound"], d["bound"] / d["cc"]) for d in used if d["cc"] > 0 and d["bound"] > 0] or [math.inf])
    r["axis_gap"] = min([d["axis_gap"] for d in used if d["axis_gap"] is not None] or [math.inf])
    r["found"] = r["best_position"] >= 0
    r["ransac_coeff"] = seen[r["best_position"]][1].astype(np.float64) if r["found"] else np.zeros(4)
    r["refined"], r["bound_n"], r["bound_d"], r["threshold_margin"] = False, 0.0, 0.0, math.inf
    if not r["found"]:
        r["coeff"], r["inliers"] = np.zeros(4), np.zeros(0, np.int32)
        return r
    m0 = seen[r["best_position"]][1]
    mask, _ = inliers_of(cloud, m0, prm["threshold"])
    r["ransac_inliers"] = np.flatnonzero(mask).astype(np.int32)
    coeff = m0
    if prm["optimize"] and mask.sum() >= 3:
        exact, r["bound_n"], r["bound_d"], r["eigenvalues"] = refine(cloud, mask, m0)
        r["coeff_exact"] = exact
        coeff = exact.astype(np.float32)
        if np.isfinite(coeff).all():
            r["refined"] = True
            mask, v = inliers_of(cloud, coeff, prm["threshold"])
            r["threshold_margin"] = float(np.abs(np.abs(v.astype(np.float64)) - float(np.float32(prm["threshold"]))).min())
        else:
            coeff = m0
    r["coeff"], r["inliers"] = coeff.astype(np.float64), np.flatnonzero(mask).astype(np.int32)
    return r
