"""Input families for the leaf filter / de-skew / re-framing tests (tests/test_pre_reference.py on the CPU, tests/test_gpu_pre_routes.py on the GPU),
and the leaf filter's route rule RESTATED -- only to size the inputs without a GPU.  The GPU test asserts the real route from the product's own
read-out (rgc_voxelgrid_route): the day somebody retunes the rule, the sizing here goes stale and that test says so."""
import numpy as np

INT_MAX = 2147483647
MAX_CELLS = 1 << 29          # rgc_params.max_cells by default
PAD_SPARSE, PAD_DENSE = 32, 8

LEAVES_IN_USE = (0.1, 0.2, 0.3, 0.5, 1.0)
LEAVES_BEYOND = (0.05, 0.15, 0.25, 0.4, 0.7, 1.1, 3.0)


def drawn_leaves(k=4, seed=20260):
    return tuple(float(np.float32(x)) for x in np.random.default_rng(seed).uniform(0.06, 2.5, k))


# ---- the route rule as csrc/rgc_api_pre.hip has it (voxelgrid_rows, vg_rows_fit), restated -----------------------------------------------
def rows_fit(div, n):
    ncell, nrows = float(div[0]) * div[1] * div[2], float(div[1]) * div[2]
    return ncell <= 2147483647.0 and ncell > 64.0 * n and nrows <= 64.0e6


def chain_route(div, n, dense):
    ss = 0 if dense else 31
    if not dense:
        nseg_max = 4.0 * n / (float(div[1]) * div[2])
        if nseg_max >= 2.0:
            ss = 3
            while ss < 30 and float((div[0] + (1 << ss) - 1) >> ss) > nseg_max:
                ss += 1
    nseg = 1 if ss >= 31 else (div[0] + (1 << ss) - 1) >> ss
    packed = (ss <= 13 or div[0] <= 8192) and n <= (1 << 27)
    return dict(leaf_buckets=int(dense), seg_shift=ss, nseg=int(nseg), packed=int(packed))


def intended_route(div, n, kept=False):
    """-> dict(kind=..., + the chain's fields): kind in copy / refused / chain; for kept=True `div` is the KEPT (measured) box, padded here;
    returns None when the kept box would not be used"""
    div = [int(d) for d in div]
    if kept:
        ps, pd = [d + 2 * PAD_SPARSE for d in div], [d + 2 * PAD_DENSE for d in div]
        if rows_fit(ps, n):
            return dict(kind="chain", **chain_route(ps, n, False))
        if float(pd[0]) * pd[1] * pd[2] <= MAX_CELLS:
            return dict(kind="chain", **chain_route(pd, n, True))
        return None
    ncell = div[0] * div[1] * div[2]
    if ncell > INT_MAX:
        return dict(kind="copy")
    if rows_fit(div, n):
        return dict(kind="chain", **chain_route(div, n, False))
    if ncell > MAX_CELLS:
        return dict(kind="refused")
    return dict(kind="chain", **chain_route(div, n, True))


def label(route):
    """the row of the issue's table a route belongs to"""
    if route is None:
        return "kept box not used"
    if route["kind"] != "chain":
        return route["kind"]
    if route["leaf_buckets"]:
        return "leaf buckets"
    ss, pk = route["seg_shift"], route["packed"]
    if ss == 31:
        return "rows packed" if pk else "rows unpacked"
    if ss == 13 and pk:
        return "seg13 packed"          # (div_x > 8192 is asserted by the case)
    return "segments packed" if pk else "segments unpacked"


# ---- clouds --------------------------------------------------------------------------------------------------------------------------
def sweep(n_az=1200, seed=3):
    import rgc_slam_amd.synth as synth
    w = synth.make_world(half_extent=40.0, seed=synth.SEED)
    sc = synth.make_scan(w, np.eye(4), n_az=n_az, seed=synth.SEED + seed)
    return np.concatenate([sc["xyz"], (sc["ring"] + 0.1 * sc["rel_time"])[:, None].astype(np.float32)], axis=1).astype(np.float32)


def box_cloud(n, lo, hi, seed, ground=0.0):
    """n points uniform in [lo, hi) (a fraction `ground` of them within 0.3 m of the floor), the two corners included so that the leaf box is the same
    for every n and seed; intensity = ring-like + fraction"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    p = rng.uniform(lo, hi, (n, 3))
    g = rng.random(n) < ground
    p[g, 2] = lo[2] + 0.3 * rng.random(int(g.sum()))
    p[0], p[1] = lo, hi - 1e-3
    out = np.empty((n, 4), np.float32)
    out[:, :3] = p
    out[:, 3] = rng.integers(0, 64, n) + rng.random(n).astype(np.float32) * 0.0999
    return out


def row_line(n_line, n_noise, leaf, seed, cube=60.0):
    """n_noise points in a cube of `cube` m, none of them in the grid row (y, z) = leaf (0, 0), plus n_line points ON that row along x, several per leaf,
    in shuffled point order: the row is one bucket of exactly n_line points when the buckets are whole rows"""
    rng = np.random.default_rng(seed)
    h = cube / 2
    noise = box_cloud(n_noise, [-h, -h, -h], [h, h, h], seed + 1)
    inv = np.float32(1) / np.float32(leaf)
    on_row = (np.floor(noise[:, 1] * inv) == 0) & (np.floor(noise[:, 2] * inv) == 0)
    on_row[:2] = False
    noise = noise[~on_row]
    line = np.empty((n_line, 4), np.float32)
    line[:, 0] = rng.uniform(-h + 0.01, h - 0.01, n_line)
    line[:, 1] = rng.uniform(0.02 * leaf, 0.9 * leaf, n_line)
    line[:, 2] = rng.uniform(0.02 * leaf, 0.9 * leaf, n_line)
    line[:, 3] = rng.random(n_line) * 100
    both = np.concatenate([noise, line])
    return np.ascontiguousarray(both[rng.permutation(len(both))])


def fullest_row(xyzi, leaf):
    """the population of the fullest (y, z) grid row, from the cloud itself"""
    inv = np.float32(1) / np.float32(leaf)
    jk = np.floor(np.asarray(xyzi, np.float32)[:, 1:3] * inv).astype(np.int64)
    _, cnt = np.unique(jk, axis=0, return_counts=True)
    return int(cnt.max())


def far_x(n, seed, pairs=True):
    """the 20 000 x 100 x 50 grid at leaf 0.1: a 2 km corridor along x.  With `pairs`, a tenth of the points are copies of others moved by exactly 8192
    leaves in x inside the same (y, z) row (leaf x taken from integer-plus-half multiples of the leaf so that the shift is exact in fp32)"""
    leaf = 0.1
    rng = np.random.default_rng(seed)
    c = box_cloud(n, [0.0, 0.0, 0.0], [2000.0, 10.0, 5.0], seed)
    if pairs:
        k = n // 10
        ix = rng.integers(1, 20000 - 8192 - 1, k)
        src = 2 + np.arange(k)
        dst = 2 + k + np.arange(k)
        c[src, 0] = ((ix + 0.5) * leaf).astype(np.float32)
        c[dst] = c[src]
        c[dst, 0] = ((ix + 8192 + 0.5) * leaf).astype(np.float32)
        c[dst, 3] += 1
        keep = np.r_[0, 1, 2 + rng.permutation(n - 2)]
        c = np.ascontiguousarray(c[keep])
    return c


def two_clusters(n, gap, seed, span=(40.0, 40.0, 10.0)):
    """two clusters `gap` (a number: along the space diagonal; or a vector) apart: the leaf box is about (gap + span) ^ 3 however few leaves are occupied"""
    rng = np.random.default_rng(seed)
    a = box_cloud(n // 2, [0, 0, 0], span, seed)
    b = box_cloud(n - n // 2, [0, 0, 0], span, seed + 1)
    b[:, :3] += np.asarray(gap, np.float32)
    c = np.concatenate([a, b])
    return np.ascontiguousarray(c[rng.permutation(n)])


def route_cases():
    """name -> dict(make(n) -> cloud, leaf, n_fresh, n_kept, want (label on a fresh context), want_kept (label on the kept, padded box), note).  n_kept is
    sized so that the PADDED box of the same cloud family takes the route the case is for."""
    sw = sweep()
    far = np.array([[900.0, 1.0, 0.5, 7.03], [901.0, -2.0, 0.2, 3.05], [899.5, 0.3, 1.0, 1.01]], np.float32)
    sw_far = np.ascontiguousarray(np.concatenate([sw, far])[np.random.default_rng(9).permutation(len(sw) + 3)])
    return {
        # the control: a 16-beam sweep.  At 0.1 m its rows outnumber its points (whole rows); at the odometer's 0.2 m it already takes short segments
        "rows_packed": dict(make=lambda n: sw[:n], leaf=0.1, n_fresh=len(sw), n_kept=len(sw) - 7, want="rows packed", want_kept="rows packed"),
        "sweep_0.2": dict(make=lambda n: sw[:n], leaf=0.2, n_fresh=len(sw), n_kept=len(sw) - 7, want="segments packed", want_kept="rows packed"),
        "leaf_buckets": dict(make=lambda n: box_cloud(n, [-3, -3, 0], [3, 3, 3], 11), leaf=0.1, n_fresh=60000, n_kept=59000, want="leaf buckets",
                             want_kept="leaf buckets"),
        # keyframe-store shape: 400 m x 400 m x 40 m at 0.4 m, most points near the ground (1000 x 1000 x 100 leaves)
        "segments_1300k": dict(make=lambda n: box_cloud(n, [-200, -200, -4], [200, 200, 36], 12, ground=0.6), leaf=0.4, n_fresh=1300000, n_kept=1300000,
                               want="segments packed", want_kept="segments packed"),
        "segments_300k": dict(make=lambda n: box_cloud(n, [-200, -200, -2], [200, 200, 18], 13, ground=0.6), leaf=0.4, n_fresh=300000, n_kept=300000,
                              want="segments packed", want_kept="segments packed"),
        "bucket_over_4095": dict(make=lambda n: row_line(6000, n - 6000, 0.2, 14), leaf=0.2, n_fresh=26000, n_kept=25000, want="rows packed",
                                 want_kept="rows packed", fullest_over=4095),
        "rows_unpacked": dict(make=lambda n: sw_far[:n] if n == len(sw_far) else np.concatenate([sw_far[:n - 3], far]), leaf=0.1, n_fresh=len(sw_far),
                              n_kept=len(sw_far) - 5, want="rows unpacked", want_kept="rows unpacked"),
        "segments_unpacked": dict(make=lambda n: far_x(n, 15), leaf=0.1, n_fresh=3000, n_kept=11000, want="segments unpacked", want_kept="segments unpacked"),
        "seg13_wide": dict(make=lambda n: far_x(n, 16), leaf=0.1, n_fresh=5000, n_kept=18000, want="seg13 packed", want_kept="seg13 packed", wide_x=True),
    }


def exact_bucket(pop, seed=21):
    """a whole-rows cloud whose fullest bucket holds exactly `pop` points"""
    return row_line(pop, 20000, 0.2, seed)


# ---- edges ---------------------------------------------------------------------------------------------------------------------------
def wall_points(leaf, seed, far=0.0):
    """coordinates fp32(m * leaf) and their nextafter neighbours either side, negative ones too; `far` moves the lattice out to where fp32 spacing is a
    visible fraction of a small leaf"""
    rng = np.random.default_rng(seed)
    m = rng.integers(-60, 60, (400, 3)).astype(np.float64)
    m[:, 0] += np.round(far / leaf)                              # (x only: the mirrored half below keeps the grid under INT_MAX leaves)
    w = (m * np.float64(np.float32(leaf))).astype(np.float32)
    lo, hi = np.nextafter(w, np.float32(-np.inf)), np.nextafter(w, np.float32(np.inf))
    xyz = np.concatenate([w, lo, hi, -w, np.nextafter(-w, np.float32(0))])
    out = np.empty((len(xyz), 4), np.float32)
    out[:, :3] = xyz
    out[:, 3] = rng.random(len(xyz)) * 64
    return np.ascontiguousarray(out[rng.permutation(len(out))])


SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097)


def sized_clouds(n, seed):
    """all points in one leaf; every point its own leaf; runs of 3 per leaf (leaf heads fall on and off the 64 / 256 / 2048-slot boundaries)"""
    rng = np.random.default_rng(seed + n)
    one = np.empty((n, 4), np.float32)
    one[:, :3] = rng.uniform(0.01, 0.19, (n, 3)); one[:, 3] = rng.random(n)
    own = np.zeros((n, 4), np.float32)
    own[:, 0] = (np.arange(n) % 97) * 0.2 + 0.1; own[:, 1] = (np.arange(n) // 97) * 0.2 + 0.1; own[:, 2] = 0.1; own[:, 3] = rng.random(n)
    own = own[rng.permutation(n)]
    runs = own.copy()
    k = np.arange(n) // 3
    runs[:, 0] = (k % 97) * 0.2 + rng.uniform(0.01, 0.19, n); runs[:, 1] = (k // 97) * 0.2 + rng.uniform(0.01, 0.19, n)
    runs = runs[rng.permutation(n)]
    return {"one_leaf": one, "own_leaf": np.ascontiguousarray(own), "runs_of_3": np.ascontiguousarray(runs)}


def strided(xyzi, stride_bytes, fill=7.5):
    """the cloud in rows of stride_bytes (12: x, y, z only); the padding holds `fill`, which no result may depend on"""
    f = stride_bytes // 4
    a = np.full((len(xyzi), f), fill, np.float32)
    c = min(f, 4)
    a[:, :c] = xyzi[:, :c]
    return a


STRIDES = (12, 16, 20, 32, 4096)


# ---- de-skew / re-framing --------------------------------------------------------------------------------------------------------------
def unit_quat(axis, angle):
    """fp64 xyzw of the rotation by `angle` about `axis`, rounded once from longdouble"""
    a = np.asarray(axis, np.longdouble)
    a = a / np.sqrt((a * a).sum())
    h = np.longdouble(angle) / 2
    return np.r_[a * np.sin(h), np.cos(h)].astype(np.float64)


def quat_with_w(w, axis=(0.3, -0.5, 0.8)):
    """a unit quaternion with the given fp64 w (the `1 - eps` switch of slerp is on w)"""
    w = np.float64(w)
    a = np.asarray(axis, np.longdouble)
    a = a / np.sqrt((a * a).sum())
    v = np.sqrt(max(np.longdouble(0), 1 - np.longdouble(w) * np.longdouble(w)))
    return np.r_[(a * v).astype(np.float64), w]


def deskew_quats():
    out = {"identity": np.array([0, 0, 0, 1.0])}
    for e in (1e-17, 1e-16, 1e-15):
        out["w=1-%g" % e] = quat_with_w(1.0 - e)
    out["small"] = unit_quat((0.1, -0.2, 1.0), 0.02)
    for ang in (0.5, 1.5, 3.1):
        out["%.1f rad" % ang] = unit_quat((0.4, 0.3, 0.85), ang)
    for k in list(out):
        if k != "identity":
            out["-(" + k + ")"] = -out[k]                       # w < 0: the same rotation
    q32 = unit_quat((0.1, -0.2, 1.0), 0.03).astype(np.float32).astype(np.float64)   # a caller's fp32 -> fp64 conversion: off unit norm by ~1e-7
    out["fp32 caller"] = q32
    out["off norm 1e-7"] = unit_quat((0.1, -0.2, 1.0), 0.03) * (1 + 1e-7)
    return out


def deskew_cloud(scale, seed, n=3000):
    """points at `scale` m; intensities ring + fraction with rings up to 127 and fractions 0, 0.05, 0.0999 and random ones"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    c = np.empty((n, 4), np.float32)
    c[:, :3] = d * scale * rng.uniform(0.5, 1.0, (n, 1))
    ring = rng.integers(0, 128, n).astype(np.float32)
    frac = np.choose(rng.integers(0, 4, n), [np.zeros(n), np.full(n, 0.05), np.full(n, 0.0999), rng.random(n) * 0.0999]).astype(np.float32)
    c[:, 3] = ring + frac
    return c


TRANSLATIONS = ((0.3, -0.05, 0.02), (300.0, -120.0, 4.0))


def random_unit_quats(k, seed):
    q = np.random.default_rng(seed).normal(size=(k, 4)).astype(np.longdouble)
    return (q / np.sqrt((q * q).sum(axis=1))[:, None]).astype(np.float64)
