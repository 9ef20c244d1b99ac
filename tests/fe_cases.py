"""Designed sweeps for the scan front-end (A1-A8): every sweep is built directly in sensor coordinates -- a point gets its ring by its
elevation, its place in the stream by its azimuth (firing order: -atan2(y, x) ascending), its range from a profile and an integer
intensity -- so that a named branch of the selection / stencil / bucket code is taken.  Nothing here draws from synth's world.

A case is a row of CASES: name -> Case(family, branch, build, minima, ...).  build() returns (raw (n, 4) float32, params, branch).
`minima` are lower bounds on the census of tests/fe_reference.py (computed from the reference restatements alone) that prove on the CPU
that the branch is reached; tests/test_fe_cases.py asserts them, tests/test_gpu_fe_routes.py holds the GPU to the oracle on the same
sweeps.  All sweeps span azimuths -2.8 .. 2.8 rad: the wrap thresholds of scanRegistration.cpp:189-203 (start - pi/2, start + 3 pi/2,
end - 3 pi/2, end + pi/2) are more than a radian away from every point, so an ulp of atan2f decides nothing (time_outliers = 0).
"""
from collections import namedtuple

import numpy as np

f32 = np.float32
O0, O1 = -2.8, 2.8

# The selection launcher's staging switch points (fe_select: lds = 8 cap + 39 (cap + 10) + 64 <= 150 KiB, cap = ring + 2 at six
# sectors per window), written down as data: (largest ring of the sweep up to and including, sectors staged per LDS window).
# A sector of more than 2048 points (a ring of 12299) is refused.
STAGING = ((3256, 6), (6512, 3), (9768, 2), (12298, 1))
RING_REFUSED = 12299
SEC_MAX = 2048


def staging_group(max_ring):
    for top, group in STAGING:
        if max_ring <= top:
            return group
    return 0   # refused


def elev_deg(ring, n_scans=16):
    """the elevation at the middle of a ring's band (the ring formulas of :141-176 inverted)"""
    if n_scans == 16:
        return 2.0 * ring - 15.0
    if n_scans == 32:
        return (ring + 0.5) * 4.0 / 3.0 - 92.0 / 3.0
    if ring == 0:
        return 1.92                                          # (its band is cut at +2 degrees, :173)
    return 2.0 - ring / 3.0 if ring <= 32 else -8.83 - (ring - 32) / 2.0


def arc(ring, m, rho, inten, n_scans=16, o0=O0, o1=O1, dz=0.0):
    """m points of one ring at azimuths o0 .. o1 (firing order), ranges rho (scalar or (m,)), integer intensities inten, height offset dz"""
    e = np.radians(elev_deg(ring, n_scans))
    ori = np.linspace(o0, o1, m)
    rho = np.broadcast_to(np.asarray(rho, np.float64), (m,))
    h = rho * np.cos(e)
    return np.stack([h * np.cos(ori), -h * np.sin(ori), rho * np.sin(e) + dz, np.broadcast_to(np.asarray(inten, np.float64), (m,))], axis=1).astype(f32)


def merge(pieces):
    """firing order: all points by ascending -atan2(y, x), rings interleaved; stable, so a ring's own order is kept"""
    P = np.concatenate([np.asarray(p, f32).reshape(-1, 4) for p in pieces])
    ori = -np.arctan2(P[:, 1].astype(np.float64), P[:, 0].astype(np.float64))
    return np.ascontiguousarray(P[np.argsort(ori, kind="stable")])


def steps(m, seed, base=10.0, every=25, levels=(0.0, 0.125, 0.25, 0.375, 0.875)):
    """plateaus of `every` points at base + a level: the edges are corners (0.125 .. 0.375 m), some jumps exceed 4 % of the range (occlusion)"""
    rng = np.random.default_rng(seed)
    lv = rng.choice(levels, size=m // every + 1)
    return base + lv[np.arange(m) // every]


def stripes(m, seed, per=9, lo=40, hi=160):
    rng = np.random.default_rng(seed + 1000)
    return np.where((np.arange(m) // per) % 2 == 0, lo, hi) + rng.integers(0, 5, m)


def floor_rho(ring, h=0.56, n_scans=16):
    return h / np.sin(np.radians(-elev_deg(ring, n_scans)))


def filler(rings, m=100, seed=0, n_scans=16, smooth=False):
    """ordinary rings: the floor (z = -0.56) under the rings that look down far enough to see it within 12 m, stepped walls at 10 m above
    (smooth: round walls of 1000 points, no corner anywhere)"""
    out = []
    for r in rings:
        if n_scans == 16 and r < 7:
            out.append(arc(r, m, floor_rho(r), stripes(m, seed + r), n_scans))
        else:
            out.append(arc(r, 1000, 10.0, 100, n_scans) if smooth else arc(r, m, steps(m, seed + r, every=12), stripes(m, seed + r), n_scans))
    return out


P16 = dict(n_scans=16, use_intensity=1)


def one_long_ring(m, ring=9, seed=0):
    return merge(filler([r for r in range(16) if r != ring], 100, seed) + [arc(ring, m, steps(m, seed + 77), stripes(m, seed + 77, per=15))])


def sawtooth(m, base=10.0, d=0.25):
    """A A B B A A B B: every point a corner (five of its ten neighbours on the other level), every level change a gap of d > sqrt(0.05) m:
    a pick suppresses its twin only, so a sector holds cnt / 2 mutually unsuppressed sharp candidates"""
    return base + d * ((np.arange(m) // 2) % 2)


def sector_bounds(start, count):
    """(sp, ep) of the six sectors of a ring that starts at `start` with `count` points (:223, :229, :478-480)"""
    S, E = start + 5, start + count - 5
    return [(S + (E - S) * j // 6, S + (E - S) * (j + 1) // 6 - 1) for j in range(6)]


# ---- near range -------------------------------------------------------------------------------------------------------------------
def _hit_range(ori, target):
    """a ring-8 point (z = 0) at azimuth ori whose fp32 range sqrt(x * x + y * y + z * z) is exactly `target`: x nudged ulp by ulp"""
    x, y = f32(float(target) * np.cos(ori)), f32(-float(target) * np.sin(ori))
    for _ in range(4000):
        r = np.sqrt(f32(f32(x * x) + f32(y * y)))
        if r == target:
            return [x, y, f32(0), f32(100)]
        x = np.nextafter(x, f32(np.inf) if r < target else f32(-np.inf))
    raise AssertionError("no fp32 point with that range")


def near_range():
    rng = np.random.default_rng(5)
    pieces = []
    for r in range(4):                                     # a floor 0.25 m under the sensor: ranges 0.97 .. 1.6 m
        pieces.append(arc(r, 120, floor_rho(r, 0.25), stripes(120, r, per=7, lo=30, hi=220)))
    for r in (9, 10, 11, 12):                              # walls at 1.0 .. 1.95 m; half of each ring jitters in height: incidence angle either side of 0.07
        m = 150
        rho = np.clip(steps(m, 40 + r, base=1.2, every=10, levels=(0.0, 0.03, 0.06, 0.3, 0.7)), 0.6, 1.95)
        dz = np.where(np.arange(m) < m // 2, 0.0, rng.uniform(-0.012, 0.012, m))
        pieces.append(arc(r, m, rho, stripes(m, r, per=7, lo=30, hi=220), dz=dz))
    two = f32(2.0)
    m = 140                                                # ring 8 (z = 0): an arc at ~2 m with range exactly 2 and its two fp32 neighbours inside it
    a8 = arc(8, m, np.where(np.arange(m) % 20 < 10, 1.97, 2.03), stripes(m, 8, per=7, lo=30, hi=220))
    ori = np.linspace(O0, O1, m)
    for k, t in ((50, np.nextafter(two, f32(0))), (51, two), (52, np.nextafter(two, f32(3))), (90, two)):
        a8[k, :3] = _hit_range(ori[k], t)[:3]
    pieces.append(a8)
    pieces += filler([13, 14, 15], 60, 3)
    return merge(pieces), dict(P16), "k_fe_stencils range < 2: incidence angle, the 0.07 gate, int smoothing, weighted inten_curvature"


# ---- exact ties -------------------------------------------------------------------------------------------------------------------
def _line(m, centre, x0=8.0, h=1.0 / 64, inten=100):
    """ring 8 (z = 0): m equispaced points on the line x = x0, y = (centre - k) * h -- dyadic, so the fp32 stencil sums are exact and the
    curvature of an interior point is exactly 0; mirror images about k = centre have bit-equal stencils"""
    k = np.arange(m)
    return np.stack([np.full(m, x0), (centre - k) * h, np.zeros(m), np.broadcast_to(inten, (m,))], axis=1).astype(f32)


def ties():
    m = 370                                                # ring 8 starts behind rings 0-7 of 100 points; E - S = 360: sectors of 60
    others = filler([r for r in range(16) if r != 8], 100, 11)
    start = 8 * 100
    sec = sector_bounds(start, m)
    c2 = (sec[2][0] + sec[2][1]) / 2.0 - start             # the centre of sector 2 (a half-integer is fine: y stays dyadic)
    L = _line(m, c2)
    # mirror pairs of equal spikes about the centre of sector 2: +-2 (inside each other's suppression reach: 3/16 m steps, gap^2 < 0.05),
    # +-12 and +-22 (tied, apart)
    for off in (2, 12, 22):
        lo = int(np.floor(c2 - off))
        for k in (lo, int(round(2 * c2 - lo))):
            L[k, 0] = 8.0 - 3.0 / 16
    # integer intensity dips of one depth in sectors 4 and 5: equal inten_curvature in the far branch
    for j in (4, 5):
        for k in range(sec[j][0] - start + 3, sec[j][1] - start - 2, 4):
            L[k, 3] = 60
    return merge(others + [L]), dict(P16), "k_fe_sort (key, index) order and the descending walk decide picks among exactly equal keys"


# ---- thresholds -------------------------------------------------------------------------------------------------------------------
def thresholds():
    others = filler([r for r in range(16) if r not in (8, 15)], 100, 21)
    # ring 8: two dyadic lines, neighbour gaps 7/32 (gap^2 = 0.0479 <= 0.05: suppression goes on) and 29/128 (0.0513 > 0.05: it stops)
    m = 120
    k = np.arange(m)
    y = np.where(k < 60, (30 - k) * (7.0 / 32), (30 - 60) * (7.0 / 32) - (k - 59) * (29.0 / 128))
    inten = np.full(m, 100)
    # intensity: inten_curvature exactly 64 / 65 / 66 (a dip of 6 and one neighbour raised by 4 / 5 / 6), steps of exactly 35 and 36 next to a pick
    for at, up in ((12, 4), (28, 5), (44, 6)):
        inten[at] = 94
        inten[at + 3] = 100 + up
    for at, nb in ((66, 55), (86, 56)):
        inten[at] = 20
        inten[at + 1] = nb
    L = np.stack([np.full(m, 8.0), y, np.zeros(m), inten], axis=1).astype(f32)
    # ring 15 (the last): range ratios either side of 0.04 -- down-steps, up-steps, and the up-step at i = cs - 6 whose mark would reach index cs
    m15 = 150
    rho = np.full(m15, 10.0)
    for at, ratio, down in ((2, 0.0401, True), (20, 0.0401, True), (40, 0.0399, True), (60, 0.0401, False), (80, 0.0399, False), (100, 0.0400, True), (120, 0.0400, False)):
        rho[at + 1:] = rho[at] / (1 + ratio) if down else rho[at] * (1 + ratio)
    rho[m15 - 5:] = rho[m15 - 6] * 1.0401                   # i = cs - 6: marks i + 1 .. i + 6, the last at index cs
    return merge(others + [L, arc(15, m15, rho, stripes(m15, 15))]), dict(P16), "values on the comparison thresholds of the stencil and selection kernels"


# ---- the curvature thresholds ------------------------------------------------------------------------------------------------------
def _ulps(lo, hi):
    """the int32 images of two positive floats: between them every integer is an fp32 value, in order"""
    return int(f32(lo).view(np.int32)), int(f32(hi).view(np.int32))


def _boundary(pred, lo, hi):
    """adjacent fp32 values (a, b), a < b, lo <= a, b <= hi, with pred(a) != pred(b); pred changes once over [lo, hi]"""
    a, b = _ulps(lo, hi)
    pa = pred(np.int32(a).view(f32))
    assert pa != pred(np.int32(b).view(f32)), "the threshold is not inside the searched interval"
    while b - a > 1:
        m = (a + b) // 2
        if pred(np.int32(m).view(f32)) == pa:
            a = m
        else:
            b = m
    return np.int32(a).view(f32), np.int32(b).view(f32)


def _tune(L, k, key, passes, want, coarse, fine):
    """Moves two coordinates of the dyadic line L (ring 8) until the restatement's `key` at point k sits as close to a threshold as fp32
    allows, on the side `want` of the comparison `passes`.  coarse / fine = (point, axis, lo, hi): first the coarse coordinate is put on
    the adjacent pair of fp32 values between which the comparison flips (bisection over the ulps), then the fine one -- whose ulp moves
    the stencil sum a tenth or less as far -- likewise, and of its pair the value on the wanted side is kept."""
    from oracle import py_frontend as pf

    def value():
        w = L[k - 5:k + 6]
        return pf.stencils(w[:, :3], w[:, 3].astype(np.int64))[key][5]
    for n_, (pt, ax, lo, hi) in enumerate((coarse, fine)):
        def pred(v):
            L[pt, ax] = v
            return bool(passes(value()))
        a, b = _boundary(pred, lo, hi)
        L[pt, ax] = a if pred(a) == want else b
        assert pred(L[pt, ax]) == want
    return value()


def curv_thresholds():
    """Candidates as close to curvature 0.1 / 0.3 and curvature2 0.3 / 0.4 as fp32 lets a sweep come, one on either side of each comparison.
    Ring 8 (z = 0) is three dyadic lines with 1/4 m between points (gap^2 = 0.0625 > 0.05: no pick suppresses a neighbour, so every
    candidate's label is decided by its own thresholds alone), whose points have curvature exactly 0 and a range curvature set by the distance:
      x = 8:  curvature2 0.4 .. 0.5 where the sensor looks at it within 30 degrees (> 0.3), a spike in HEIGHT sets the curvature alone: corner iff curvature > 0.1;
      x = 16: curvature2 ~ 0.24; a spike in height makes the curvature 0.18, a step in x moves curvature2 across 0.3 (corner or plane)
              or, without the height spike, across 0.4 (plane or nothing);
      x = 32: curvature2 ~ 0.08 (< 0.4), a spike in height moves the curvature across 0.3: plane or nothing.
    The curvature is (dZ^2) * f32(2 / (1 + range / 20)) with dZ a sum rounded at 3e-8: both fp32 neighbours of a threshold are usually
    not both attainable; curvature2 is a sum of ranges whose own ulp is 1e-6 at 8 .. 16 m.  The census counts what was reached within
    1e-7 (curvature) and 5e-6 (curvature2) of each threshold, on either side, with the label the comparison decides."""
    h = 0.25
    A = np.stack([np.full(35, 8.0), 9.5 - h * np.arange(35), np.zeros(35), np.full(35, 100.0)], axis=1)          # ori -0.871 .. -0.124
    C = np.stack([np.full(48, 16.0), 1.75 - h * np.arange(48), np.zeros(48), np.full(48, 100.0)], axis=1)        # ori -0.109 .. 0.558
    B = np.stack([np.full(48, 32.0), -20.25 - h * np.arange(48), np.zeros(48), np.full(48, 100.0)], axis=1)      # ori 0.564 .. 0.791
    L = np.concatenate([A, C, B]).astype(f32)
    base = 1.0e-4
    gt = lambda t: (lambda v: float(v) > t)
    lt = lambda t: (lambda v: float(v) < t)
    zs = lambda k, lo, hi: ((k, 2, lo, hi), (k + 1, 2, 0.25 * base, 4 * base))
    for k in (22, 29, 35 + 8, 35 + 20, 35 + 32, 35 + 42, 83 + 10, 83 + 24):
        L[k + 1, 2] = base                                 # the fine coordinate starts in the middle of its interval
    for k, want in ((22, False), (29, True)):              # x = 8: curvature > 0.1
        _tune(L, k, "curvature", gt(0.1), want, *zs(k, 0.01, 0.1))
    for k, want in ((83 + 10, True), (83 + 24, False)):    # x = 32: curvature < 0.3
        _tune(L, k, "curvature", lt(0.3), want, *zs(k, 0.01, 0.2))
    for k, want in ((35 + 8, False), (35 + 20, True)):     # x = 16: curvature 0.18 from the height spike, curvature2 > 0.3 from the step in x
        L[k, 2] = 0.04
        L[k + 1, 2] = 0.0
        _tune(L, k, "curvature2", gt(0.3), want, (k, 0, 15.9, 16.0), (k + 1, 0, 15.99, 16.01))
    for k, want in ((35 + 32, True), (35 + 42, False)):    # x = 16: curvature2 < 0.4, curvature small
        L[k + 1, 2] = 0.0
        _tune(L, k, "curvature2", lt(0.4), want, (k, 0, 15.9, 16.0), (k + 1, 0, 15.99, 16.01))
    return (merge(filler([r for r in range(16) if r != 8], 100, 23) + [L]), dict(P16),
            "curvature within an fp32 step or two of 0.1 / 0.3, curvature2 within 5e-6 of 0.3 / 0.4, either side, each deciding a label")


# ---- quotas and add_inten ---------------------------------------------------------------------------------------------------------
def quota_sharp():
    m = 600
    return (merge(filler([r for r in range(16) if r != 9], 100, 31) + [arc(9, m, sawtooth(m), 100)]), dict(P16),
            "sharp quota: the 21st pick labelled 1 without a slot, the 22nd untouched")


def quota_flat():
    m = 3000
    return merge(filler([r for r in range(16) if r != 9], 100, 32) + [arc(9, m, 10.0, 100)]), dict(P16), "flat quota: the 41st candidate ends the pass"


def quota_inten():
    m = 600
    inten = np.where((np.arange(m) // 2) % 2 == 0, 40, 160)
    return (merge(filler([r for r in range(16) if r != 9], 100, 33, smooth=True) + [arc(9, m, 10.0, inten)]), dict(P16),
            "intensity quota: 21st labelled 1, 22nd untouched; no corners, so n_sharp_own / n_flat < 0.3 and the intensity corners are appended")


def ratio_high():
    """many corners, few planes: n_sharp_own / n_flat >= 0.3, the intensity corners are NOT appended"""
    pieces = [arc(r, 200, sawtooth(200, base=20.0), np.where((np.arange(200) // 2) % 2 == 0, 40, 160)) for r in range(15)]
    pieces.append(arc(15, 2000, 20.0, 100))                # the planes: one round wall
    return merge(pieces), dict(P16), "add_inten false: n_sharp_own / n_flat >= 0.3"


def no_flat():
    pieces = [arc(r, 200, sawtooth(200, base=20.0), np.where((np.arange(200) // 2) % 2 == 0, 40, 160)) for r in range(16)]
    return merge(pieces), dict(P16), "n_flat == 0: the ratio divides by zero and nothing is appended"


def no_intensity():
    raw, _, _ = quota_inten()
    return raw, dict(n_scans=16, use_intensity=0), "use_intensity = 0: intensity corners found but not appended"


# ---- sector start-over ------------------------------------------------------------------------------------------------------------
def redo_sharp_flat():
    """rings of 130 points (sectors of 20): a spike two points before each sector border and a weaker one right behind it, 3/16 and 2/16 m
    deep with 4 cm between points: the serial walk's pick in sector j - 1 suppresses what sector j alone would pick first"""
    pieces = filler(range(7), 100, 41)
    for r in range(7, 16):
        m = 130
        rho = np.full(m, 8.0)
        for (sp, ep) in sector_bounds(0, m)[1:]:
            rho[sp - 2] -= 3.0 / 16
            rho[sp + 1] -= 2.0 / 16
        pieces.append(arc(r, m, rho, 100, o0=-0.4, o1=0.4))
    return merge(pieces), dict(P16), "six sectors at once: a sector starts over after its predecessor's mark lands on one of its sharp / flat picks"


def redo_inten():
    """the same for the intensity flags alone: intensity dips of 30 before and 20 behind each border, on rings whose points zig-zag 6 cm
    in HEIGHT (A A B B): curvature >= 0.3 with a range curvature <= 0.3 -- neither corner nor plane, so no sharp / flat pick exists there"""
    pieces = filler(range(7), 100, 42)
    for r in range(7, 16):
        m = 130
        inten = np.full(m, 100)
        for (sp, ep) in sector_bounds(0, m)[1:]:
            inten[sp - 2] -= 30
            inten[sp + 1] -= 20
        pieces.append(arc(r, m, 8.0, inten, o0=-0.4, o1=0.4, dz=0.06 * ((np.arange(m) // 2) % 2)))
    return merge(pieces), dict(P16), "six sectors at once: a sector starts over after a mark lands on one of its intensity picks"


# ---- ring sizes -------------------------------------------------------------------------------------------------------------------
def rings_small():
    sizes = {8: 19, 9: 20, 10: 21, 11: 81, 12: 82}
    pieces = filler([r for r in range(16) if r not in sizes], 100, 51)
    for r, m in sizes.items():
        pieces.append(arc(r, m, steps(m, 60 + r, every=6), stripes(m, 60 + r, per=5)))
    return merge(pieces), dict(P16), "rings of 19 / 20 / 21 points (E - S = 9, 10, 11) and of 81 / 82 (a sector of 11 / 12: serial or six at once)"


def ring_of(m):
    return lambda: (one_long_ring(m, seed=m % 97), dict(P16), "largest ring %d: %d sectors staged per window" % (m, staging_group(m)))


def rings_64():
    pieces = []
    for r in range(51):
        m = 60 + (r % 5)
        pieces.append(arc(r, m, steps(m, 70 + r, every=8), stripes(m, 70 + r, per=6), n_scans=64))
    return merge(pieces), dict(n_scans=64, use_intensity=1), "64 rings (51 in use): the 64-column ring histogram and 306 sectors"


# ---- bucket and stencil counts ----------------------------------------------------------------------------------------------------
def total_n(n):
    def build():
        per = [n // 3, n // 3, n - 2 * (n // 3)]
        pieces = [arc(r, m, floor_rho(r) if r < 7 else steps(m, n + r, every=9), stripes(m, n + r, per=6)) for r, m in zip((2, 8, 12), per)]
        return merge(pieces), dict(P16), "n = %d: %d blocks of 256" % (n, (n + 255) // 256)
    return build


def blocks_n(n):
    def build():
        per = [n // 16] * 16
        per[9] += n - sum(per)
        pieces = [arc(r, m, floor_rho(r) if r < 7 else steps(m, n + r, every=11), stripes(m, n + r)) for r, m in enumerate(per)]
        return merge(pieces), dict(P16), "n = %d: %d blocks, the 16 chunks of the histogram scan" % (n, (n + 255) // 256)
    return build


def one_ring():
    return arc(9, 500, steps(500, 81, every=10), stripes(500, 81)), dict(P16), "all points in one ring"


def no_ground_rings():
    return merge(filler(range(7, 16), 100, 82)), dict(P16), "rings 0-6 empty: no ground"


def ground_10_11():
    pieces = [arc(0, 10, floor_rho(0), 100), arc(1, 11, floor_rho(1), 100)] + filler(range(7, 16), 100, 83)
    return merge(pieces), dict(P16), "ground rings of 10 (skipped) and 11 points (one seed column)"


def outside_fan():
    pieces = filler(range(16), 100, 84)
    e = np.radians(21.0)
    for sgn in (-1, 1):                                    # +-21 degrees: outside the 16-beam fan (ring = -1), interleaved in azimuth
        ori = np.linspace(O0 + 0.01, O1 - 0.01, 333)
        pieces.append(np.stack([6 * np.cos(e) * np.cos(ori), -6 * np.cos(e) * np.sin(ori), np.full(333, sgn * 6 * np.sin(e)), np.full(333, 50.0)], axis=1))
    return merge(pieces), dict(P16), "points outside the beam fan (ring = -1) interleaved with kept points"


def lanes(first, last_lane):
    """dropped points (inside min_range) in front of and behind the sweep so that the first kept point sits at index `first` and the last on
    lane `last_lane` of its wave"""
    def build():
        body = merge(filler(range(16), 40, 85))
        junk = np.array([[0.1, 0.1, 0.0, 5.0]], f32)
        while (first + len(body) - 1) % 64 != last_lane:
            body = body[:-1]
        raw = np.concatenate([np.repeat(junk, first, 0), body, np.repeat(junk, 70, 0)])
        return raw, dict(P16), "first kept point at index %d (lane %d), last kept on lane %d" % (first, first % 64, last_lane)
    return build


def ring_starts():
    counts = [246, 261, 261, 261, 261] + [100] * 11          # ring starts 246 = 256 - 10, 507 = 512 - 5, 768, 1029 = 1024 + 5, 1290 = 1280 + 10
    pieces = [arc(r, m, floor_rho(r) if r < 7 else steps(m, 86 + r, every=12), stripes(m, 86 + r)) for r, m in enumerate(counts)]
    return merge(pieces), dict(P16), "ring starts at 256 m + {-10, -5, 0, 5, 10}: the stencil tile's halo"


def ground_collinear():
    """the ground set on one straight line (ring 0 only, a dyadic line at z = -0.5): the plane through it is not determined"""
    m = 40
    k = np.arange(m)
    L = np.stack([np.full(m, 2.0), (20 - k) / 32.0, np.full(m, -0.5625), np.full(m, 100.0)], axis=1)
    return merge([L] + filler(range(7, 16), 100, 87)), dict(P16), "a collinear ground set: two equal smallest eigenvalues"


def ground_single():
    """the ground set one repeated point"""
    L = np.tile(np.array([[2.5, -0.25, -0.6875, 100.0]]), (30, 1))
    return merge([L] + filler(range(7, 16), 100, 88)), dict(P16), "a ground set that is one repeated point: zero covariance"


# ---- speculative sizing (cloud=False from the second sweep on): largest rings around prev + prev / 4 + 64 -------------------------
def spec_ring(m, seed):
    return lambda: (merge(filler([r for r in range(16) if r != 9], 100, seed) + [arc(9, m, steps(m, seed + 5), stripes(m, seed + 5))]), dict(P16),
                    "largest ring %d on the speculative path" % m)


def empty():
    return np.full((300, 4), 1000.0, f32), dict(P16), "every point beyond max_range: an empty sweep"


Case = namedtuple("Case", "family build minima refused")


def _c(family, build, minima=None, refused=False):
    return Case(family, build, minima or {}, refused)


# minima: census key -> the least the reference must count for the case to do its job (tests/fe_reference.py: census)
CASES = {
    "near_range": _c("near", near_range, dict(near=900, near_gate=150, near_no_gate=150, smoothed=150, near_inten_features=5, range_eq_2=1, range_below_2=1, range_above_2=1)),
    "ties": _c("ties", ties, dict(tied_flat=200, tied_sharp=6, tied_inten=10, tie_order_decides=2)),
    "curv_thresholds": _c("thresholds", curv_thresholds, dict(curv_01_lo=1, curv_01_hi=1, curv_03_lo=1, curv_03_hi=1, curv2_03_lo=1, curv2_03_hi=1, curv2_04_lo=1, curv2_04_hi=1, curv_03_adjacent=1)),
    "thresholds": _c("thresholds", thresholds, dict(icurv_64=1, icurv_65=1, icurv_66=1, step_35=1, step_36=1, gap_below=40, gap_above=40, occl_near_004=7, occl_mark_at_cs=1, occl_cross_ring=1)),
    "quota_sharp": _c("quota", quota_sharp, dict(sharp_quota_cut=1, sharp_label_1=1)),
    "quota_flat": _c("quota", quota_flat, dict(flat_quota_cut=1)),
    "quota_inten": _c("quota", quota_inten, dict(inten_quota_cut=1, inten_label_1=1, add_inten=1, tied_inten=100, tie_order_decides=1)),
    "ratio_high": _c("quota", ratio_high, dict(ratio_ge_03_with_flat=1)),
    "no_flat": _c("quota", no_flat, dict(n_flat_zero=1, inten_found_not_added=1)),
    "no_intensity": _c("quota", no_intensity, dict(inten_found_not_added=1)),
    "redo_sharp_flat": _c("redo", redo_sharp_flat, dict(redo_label=9, parallel_rings=9)),
    "redo_inten": _c("redo", redo_inten, dict(redo_inten_only=9, parallel_rings=9)),
    "rings_small": _c("rings", rings_small, dict(ring_19=1, ring_20=1, ring_21=1, ring_81=1, ring_82=1)),
    "ring_3256": _c("rings", ring_of(3256), dict(max_ring=3256, group_6=1)),
    "ring_3257": _c("rings", ring_of(3257), dict(max_ring=3257, group_3=1)),
    "ring_6512": _c("rings", ring_of(6512), dict(max_ring=6512, group_3=1)),
    "ring_6513": _c("rings", ring_of(6513), dict(max_ring=6513, group_2=1)),
    "ring_9768": _c("rings", ring_of(9768), dict(max_ring=9768, group_2=1)),
    "ring_9769": _c("rings", ring_of(9769), dict(max_ring=9769, group_1=1)),
    "ring_12298": _c("rings", ring_of(12298), dict(max_ring=12298, group_1=1, max_sector=2048)),
    "ring_12299": _c("rings", ring_of(12299), dict(max_ring=12299, max_sector=2049), refused=True),
    "rings_64": _c("rings", rings_64, dict(rings_in_use=51)),
    "n_255": _c("counts", total_n(255), dict(n_cloud=255)),
    "n_256": _c("counts", total_n(256), dict(n_cloud=256)),
    "n_257": _c("counts", total_n(257), dict(n_cloud=257)),
    "blocks_15": _c("counts", blocks_n(3840), dict(n_cloud=3840)),
    "blocks_16": _c("counts", blocks_n(4096), dict(n_cloud=4096)),
    "blocks_17": _c("counts", blocks_n(4097), dict(n_cloud=4097)),
    "one_ring": _c("counts", one_ring, dict(rings_in_use=1)),
    "no_ground_rings": _c("counts", no_ground_rings, dict(no_ground=1)),
    "ground_10_11": _c("counts", ground_10_11, dict(ground_pts=1)),
    "outside_fan": _c("counts", outside_fan, dict(outside_fan=666)),
    "lanes_0_63": _c("counts", lanes(64, 63), dict(first_lane_0=1, last_lane_63=1)),
    "lanes_63_0": _c("counts", lanes(127, 0), dict(first_lane_63=1, last_lane_0=1)),
    "ring_starts": _c("counts", ring_starts, dict(ring_start_tiles=5)),
    "spec_1000": _c("spec", spec_ring(1000, 91), dict(max_ring=1000)),
    "spec_1326": _c("spec", spec_ring(1326, 92), dict(max_ring=1326)),      # after 1000: the largest ring the guessed window holds (spec_route)
    "spec_1327": _c("spec", spec_ring(1327, 93), dict(max_ring=1327)),      # one more: flag bit 2, the sweep is done again
    "spec_3000": _c("spec", spec_ring(3000, 94), dict(max_ring=3000, group_6=1)),   # after itself: guessed 3814 -> staged three sectors at a time
    "empty": _c("spec", empty, dict(empty=1)),
    "ground_collinear": _c("counts", ground_collinear, dict(ground_pts=10, ground_degenerate=1)),
    "ground_single": _c("counts", ground_single, dict(ground_pts=10, ground_degenerate=1)),
}

# ---- the speculative path as the launcher decides it, restated as a model over ring counts ------------------------------------------
def select_refuses(ring_counts, max_ring):
    """k_fe_select's `oversize` for a launch sized by max_ring (fe_select: group and sec_cap from max_ring; the kernel: a staging window of
    `group` sectors holds more than sec_cap points, or a sector more than SEC_MAX)"""
    group, cap = 6, 0
    while True:
        cap = min((max_ring * group + 5) // 6 + 2, SEC_MAX * group)
        if 8 * cap + 39 * (cap + 10) + 64 <= 150 * 1024 or group == 1:
            break
        group = {6: 3, 3: 2, 2: 1}[group]
    for m in ring_counts:
        if m - 10 < 10:
            continue
        b = sector_bounds(0, int(m))
        if max(ep - sp + 1 for sp, ep in b) > SEC_MAX:
            return True, group
        for j0 in range(0, 6, group):
            if b[j0 + group - 1][1] - b[j0][0] + 1 > cap:
                return True, group
    return False, group


def spec_route(state, n_scans, ring_counts, n_raw):
    """frontend_impl with cloud = NULL: state = (n_scans, largest ring) of the last finished sweep or None.  Returns (route, group, state):
    'sync' (no guess to size from), 'spec' (sized from the guess prev + prev / 4 + 64, the window holds), 'fallback' (the guessed window
    is too small: ring - 10 > guess + 2 at six sectors per window, i.e. ring >= guess + 13; the sweep is done again synchronously),
    'refused' (the synchronous launch refuses too), 'empty'"""
    biggest = int(max(ring_counts)) if len(ring_counts) else 0
    spec = state is not None and state[0] == n_scans and state[1] > 0
    if biggest == 0:
        return "empty", 0, state
    route = "sync"
    if spec:
        over, group = select_refuses(ring_counts, min(n_raw, state[1] + state[1] // 4 + 64))
        if not over:
            return "spec", group, (n_scans, biggest)
        route = "fallback"
    over, group = select_refuses(ring_counts, biggest)
    if over:
        return "refused", 0, ((n_scans, 0) if spec else state)
    return route, group, (n_scans, biggest)


# what a second context is fed through the speculative path (cloud=False), in this order, starting behind one spec_1000 sweep; "@64"
# switches it to 64 rings for that sweep.  Next to each: the route and the sectors per staging window that spec_route derives (asserted
# without a GPU by tests/test_fe_cases.py): the guess after 1000 is 1314, a window of 1316 points, so 1326 (E - S = 1316) is the last
# ring that stays speculative and 1327 the first that falls back; 3000 after 3000 is staged three sectors at a time where the
# synchronous path stages six.
SPEC_SEQUENCE = (("spec_1000", "spec", 6), ("spec_1326", "spec", 6), ("spec_1000", "spec", 6), ("spec_1327", "fallback", 6), ("empty", "empty", 0),
                 ("spec_1000", "spec", 6), ("spec_3000", "fallback", 6), ("spec_3000", "spec", 3), ("ring_3257", "spec", 3), ("rings_64@64", "sync", 6),
                 ("spec_1000", "sync", 6), ("ring_12299", "refused", 0), ("spec_1000", "sync", 6), ("spec_1326", "spec", 6))

_built = {}


def get(name):
    """(raw, params, branch) of a case, built once"""
    if name not in _built:
        raw, prm, branch = CASES[name].build()
        raw = np.ascontiguousarray(raw, f32)
        raw.setflags(write=False)
        _built[name] = (raw, prm, branch)
    return _built[name]
