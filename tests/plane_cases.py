"""Designed inputs of RANSAC plane segmentation (rgc_plane_segment) for tests/test_plane_reference.py (no GPU: what each case contains, from the reference
alone) and tests/test_gpu_plane.py (the library against the reference).  A case: the cloud, the parameters, the caller's samples (None: the generated
stream), `expect` (values the reference must give EXACTLY: the situation the case was designed for) and `minima` (lower bounds on reference values).

Coordinates of the designed clouds are dyadic, so a designed triple's model is exact: (0,0,0)-(1,0,0)-(0,1,0) gives (0, 0, 1, 0) and so on.

  size_N        N = 3, 4, 63, 64, 65, 255, 256, 257 (one point either side of the 256-point tile of a scan-sized cloud), 1023 .. 1025, 65535 .. 65537 (either
                side of the change to four points per thread, whose tile is 1024 points), 66559 .. 66561 (either side of a 1024-point tile):
                a noisy plane in uniform clutter, caller's samples
  many_groups   200 000 points: many workgroups add into the same counters; the generated stream
  threshold     the plane z = 0 from a dyadic triple, threshold 2^-4: points AT |z| = 2^-4 are excluded (strict), points at the next float32 below are in
  tie, tie_rev  two positions tie on the count: the earlier one wins
  last_of_7, first_of_8, last_of_64, first_of_65   the best model is the last position of a batch / the first of the next one (batches of 7 and 64)
  adaptive_90   90 % inliers: the adaptive stop, in the middle of a batch
  max_iter      max_iterations reached;  stream_end: the caller's samples run out first
  all_invalid   a stream of collinear and coincident triples only (duplicated points included); line: a cloud ON a line under the generated stream
  axis_none     an axis constraint that rejects every position;  axis_some: one that accepts exactly the positions within eps_angle
  scan_sS       a 30 000-point synthetic LiDAR scan (synth), the generated stream, seeds 1, 2, 3"""
import math

import numpy as np

import plane_reference as pr

SIZES = (3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537, 66559, 66560, 66561)
BATCHES = (1, 7, 64, 0)


def _case(name, cloud, prm, samples=None, expect=None, minima=None):
    return dict(name=name, cloud=np.ascontiguousarray(cloud, np.float32), prm=prm, samples=None if samples is None else np.ascontiguousarray(samples, np.int32).reshape(-1, 3),
                expect=expect or {}, minima=minima or {})


def _noisy_plane(n, seed, inlier_share=0.6):
    """a plane z ~ 0 (|z| < 2^-5 in steps of 2^-10) in uniform clutter, everything dyadic, in a fixed shuffled order"""
    rng = np.random.default_rng(seed)
    m = int(round(n * inlier_share))
    a = np.empty((n, 3), np.float64)
    a[:m, :2] = rng.integers(-128, 128, (m, 2)) / 16.0
    a[:m, 2] = rng.integers(-31, 32, m) / 1024.0
    a[m:] = rng.integers(-2048, 2048, (n - m, 3)) / 256.0
    return a[rng.permutation(n)].astype(np.float32)


def _triples(n, count, seed):
    rng = np.random.default_rng(seed)
    return np.array([rng.choice(n, 3, replace=False) for _ in range(count)], np.int32)


# ---- the designed cloud of the batch-boundary, tie, stop and axis cases: three exact planes and clutter ----
def _three_planes():
    rng = np.random.default_rng(5)
    A = [(1, 1, 0), (2, 1, 0), (1, 2, 0)] + [(x, y, 0) for x, y in rng.integers(1, 40, (27, 2))]            # 30 on z = 0, away from the other planes
    B = [(0, 1, 1), (0, 2, 1), (0, 1, 2)] + [(0, y, z) for y, z in rng.integers(1, 40, (17, 2))]            # 20 on x = 0
    Cc = [(1, 0, 1), (2, 0, 1), (1, 0, 2)] + [(x, 0, z) for x, z in rng.integers(1, 40, (7, 2))]            # 10 on y = 0
    noise = [tuple(v) for v in rng.integers(41, 90, (40, 3))]
    return np.array(A + B + Cc + noise, np.float64) / 4.0, (0, 1, 2), (30, 31, 32), (50, 51, 52)


def _boundary_cases():
    cloud, A, B, Cc = _three_planes()
    out = []
    for name, at, length in (("last_of_7", 6, 20), ("first_of_8", 7, 20), ("last_of_64", 63, 70), ("first_of_65", 64, 70)):
        s = [Cc if t % 2 else B for t in range(length)]
        s[at] = A
        out.append(_case(name, cloud, pr.params(0.125, max_iterations=200), s, expect=dict(best_position=at, best_count=30, positions=length, skipped=0)))
    t = np.concatenate([cloud[:20], cloud[30:50]])                      # 20 on z = 0 and 20 on x = 0: the counts tie
    out.append(_case("tie", t, pr.params(0.125, max_iterations=2), [(0, 1, 2), (20, 21, 22), (0, 1, 2)], expect=dict(best_position=0, best_count=20, iterations=2, positions=2)))
    out.append(_case("tie_rev", t, pr.params(0.125, max_iterations=2), [(20, 21, 22), (0, 1, 2), (0, 1, 2)], expect=dict(best_position=0, best_count=20, iterations=2, positions=2)))
    out.append(_case("max_iter", cloud, pr.params(0.125, max_iterations=3), [Cc, B, Cc, A, A, A, A, A, A, A], expect=dict(iterations=3, positions=3, best_position=1, best_count=20)))
    out.append(_case("stream_end", cloud, pr.params(0.125, max_iterations=50), [Cc, Cc, B, A, B], expect=dict(iterations=5, positions=5, best_position=3)))
    # the axis constraint: A's normal is z, B's x, Cc's y; the tilted triples have normals atan(1/8) = 0.124 and atan(1/2) = 0.464 rad from z
    tilt = np.array([(0, 0, 0), (8, 0, 1), (0, 8, 0), (8, 0, 4)], np.float64) / 4.0
    ax = np.concatenate([cloud, tilt])
    n0 = len(cloud)
    near, far = (n0, n0 + 1, n0 + 2), (n0, n0 + 3, n0 + 2)
    out.append(_case("axis_none", ax, pr.params(0.125, max_iterations=50, model=pr.PERPENDICULAR, axis=(0, 3, 0), eps_angle=0.1), [A, B, far, near, A, B],
                     expect=dict(skipped=6, iterations=0, best_position=-1, positions=6)))
    out.append(_case("axis_some", ax, pr.params(0.125, max_iterations=50, model=pr.PERPENDICULAR, axis=(0, 0, 2), eps_angle=0.2), [B, far, near, Cc, A, B, far],
                     expect=dict(skipped=5, iterations=2, best_position=4, best_count=32, positions=7)))
    return out


def _threshold_case():
    t, under = np.float32(2.0 ** -4), np.nextafter(np.float32(2.0 ** -4), np.float32(0))
    pts = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
    for k in range(6):
        s = 1.0 if k % 2 else -1.0
        pts += [(k + 2, k * 0.5, s * float(t)), (k + 2, -k * 0.25, s * float(under)), (-k - 1, 3, s * float(np.nextafter(t, np.float32(1)))), (k, k, 0.5)]
    return _case("threshold", pts, pr.params(2.0 ** -4, max_iterations=5), [(0, 1, 2)], expect=dict(best_position=0, best_count=9, positions=1, iterations=1))


def _adaptive_case():
    cloud = np.concatenate([_noisy_plane(400, 17, 0.9), np.array([(-8, -8, 0), (8, -8, 0), (0, 8, 0)], np.float32)])   # three anchors ON z = 0: the exact model (0, 0, 1, 0)
    off = np.flatnonzero(np.abs(cloud[:, 2]) > 1.0)
    anchors = [(400, 401, 402), (401, 402, 400), (402, 400, 401)]
    s = [tuple(int(v) for v in off[:3])] + anchors * 4
    # 363 of 403 points: w = 0.9007, k = log(0.01) / log(1 - w^3) = 3.51: the loop stops behind its fourth position
    return _case("adaptive_90", cloud, pr.params(0.05, max_iterations=50), s, expect=dict(iterations=4, positions=4, best_position=1, best_count=363))


def _invalid_cases():
    line = np.array([(k, 0, 0) for k in range(8)] + [(3, 0, 0), (3, 0, 0), (5, 5, 5), (1, 2, 3), (7, 1, 2)], np.float64) / 2.0
    s = [(0, 1, 2), (7, 3, 5), (3, 8, 9), (3, 8, 1), (0, 7, 4), (8, 9, 10)]                  # collinear, coincident (three copies of one point), two copies and a third point
    out = [_case("all_invalid", line, pr.params(0.25, max_iterations=50), s, expect=dict(skipped=6, iterations=0, best_position=-1, positions=6))]
    on_line = np.array([(k, 2 * k, -k) for k in range(-40, 41)], np.float64) / 8.0
    out.append(_case("line", on_line, pr.params(0.25, max_iterations=4, seed=9), None, expect=dict(skipped=40, iterations=0, best_position=-1, positions=40)))
    return out


def all_cases():
    out = []
    for n in SIZES:
        cloud = _noisy_plane(n, 100 + n)
        s = [(0, 1, 2), (1, 2, 0), (2, 0, 1)] if n == 3 else _triples(n, 12, n)
        out.append(_case("size_%d" % n, cloud, pr.params(0.05, max_iterations=8), s))
    out.append(_case("many_groups", _noisy_plane(200000, 7, 0.5), pr.params(0.05, max_iterations=20, seed=4), None, minima=dict(best_count=40000)))
    return out + [_threshold_case(), _adaptive_case()] + _boundary_cases() + _invalid_cases()


def scan_cases():
    from rgc_slam_amd import synth
    world, _ = synth.make_world_and_map(30000)
    scan = np.ascontiguousarray(synth.make_scan_n(world, np.eye(4), 30000)["xyz"], np.float32)
    return [_case("scan_s%d" % s, scan, pr.params(0.2, max_iterations=50, seed=s), None, minima=dict(best_count=3000)) for s in (1, 2, 3)]


CASES = {c["name"]: c for c in all_cases()}
SCANS = ("scan_s1", "scan_s2", "scan_s3")
_cache = {}


def case(name):
    if name not in CASES:
        CASES.update({c["name"]: c for c in scan_cases()})
    return CASES[name]


def ref(name, optimize=1):
    """the reference of a case, computed once and shared (the sequential definition)"""
    if (name, optimize) not in _cache:
        c = case(name)
        _cache[(name, optimize)] = pr.run(c["cloud"], dict(c["prm"], optimize=optimize), c["samples"])
    return _cache[(name, optimize)]


def tolerances(r, cloud):
    """what a reported refined coefficient may differ from the longdouble reference by -- the derived bound of plane_reference.refine plus the rounding of
    the result to float32 (2^-24 relative) -- and the distance from the threshold below which a point's membership is not decided by the reference"""
    e = r["coeff_exact"]
    tol = np.array([r["bound_n"] + 2.0 ** -24 * abs(e[k]) for k in range(3)] + [r["bound_d"] + 2.0 ** -24 * abs(e[3])])
    extent = float(np.abs(cloud[:, :3]).max()) + 1.0
    undecided = 4.0 * (r["bound_n"] + 2.0 ** -22) * extent + r["bound_d"]
    return tol, undecided


UNDECIDED = ("many_groups", "size_65536", "size_66561")


def decided(name):
    """whether the reference decides the RE-SELECTED inlier set of a refined case: no point lies nearer to the threshold than `undecided` (tolerances).
    Every designed case and scan must be, except UNDECIDED, whose nearest point lies a few 1e-6 m from it (tests/test_plane_reference.py asserts both)"""
    r = ref(name, 1)
    return not r["refined"] or r["threshold_margin"] > tolerances(r, case(name)["cloud"])[1]


def two_pass_case():
    """2 200 001 points: more 1024-point tiles than the scoring kernel's grid cap of 2048 workgroups, so that workgroups take a second tile and still flush
    once; caller's samples, no refinement (the counts are what this case is about).  Not in CASES: only tests/test_gpu_plane.py's count test uses it"""
    n = 2200001
    return _case("two_pass", _noisy_plane(n, 23, 0.5), pr.params(0.05, max_iterations=5, optimize=0), _triples(n, 5, 23))


def guards(r):
    """the conditions under which equality with the reference is decidable: no `iterations >= k` within 1e-12 relative of equality, no triple within a
    factor 4 of the collinearity bound (exact zeros aside), no |n.a| within 1e-9 of cos(eps_angle)"""
    return r["k_margin"] > 1e-12 and r["collinear_factor"] > 4.0 and r["axis_gap"] > 1e-9
