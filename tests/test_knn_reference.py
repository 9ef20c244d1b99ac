"""The CPU oracle's exact k-NN and covariances against tests/knn_reference.py (numpy / scipy) at EVERY k the API accepts (2..32).

The GPU tests of tests/test_gpu_knn_k_range.py lean on the oracle at k values its own pin (tests/fuzz/fuzz_oracle_pin.py: k = 10 / 20 / 25,
neighbour sets allowed to differ on n / 200 rows) never saw.  Here the oracle must give the reference's neighbour rows exactly -- the same
indices in the same (key, index) order, the fp32 keys bit for bit -- and its covariances to 1e-12 (NONE, MIN_EIG) and 1e-9 (PLANE, on rows
whose eigengap defines the normal) on clouds built to hit the rank, tie and size edges.  No GPU."""
import numpy as np
import pytest

import knn_reference as kr

K_ALL = list(range(2, 33))


def _lattice(rng):
    """anisotropic lattice (0.25 / 0.27 / 0.31) with 120 exact duplicates: many candidates at exactly the k-th key"""
    g = np.stack(np.meshgrid(np.arange(14), np.arange(12), np.arange(6), indexing="ij"), axis=-1).reshape(-1, 3)
    g = (g * np.array([0.25, 0.27, 0.31])).astype(np.float32)
    pts = np.concatenate([g, g[rng.choice(len(g), 120, replace=False)]])
    return pts[rng.permutation(len(pts))] + np.float32([3.0, -2.0, 0.5])


def _clump(rng):
    """a dense clump (800 points in 0.2 m) inside a sparse field (1 700 points in 40 m)"""
    clump = rng.normal(0.0, 0.05, (800, 3)) + [5.0, 5.0, 1.0]
    field = rng.uniform(-20.0, 20.0, (1700, 3))
    pts = np.concatenate([clump, field]).astype(np.float32)
    return pts[rng.permutation(len(pts))]


def _pole(base, rng, n=60):
    """an exactly collinear pole (constant fp32 x and y) inside a map, in a 2 m clearing: rank-1 neighbourhoods"""
    z = np.linspace(0.0, 3.0, n)
    pole = np.stack([np.full(n, 2.375), np.full(n, -1.625), z], axis=1).astype(np.float32)
    clear = np.hypot(base[:, 0] - 2.375, base[:, 1] + 1.625) > 2.0
    pts = np.concatenate([base[clear], pole])
    return pts[rng.permutation(len(pts))]


def _origin_copies(base, rng, k):
    """k + 5 copies of (0, 0, 0) -- invalid LiDAR returns -- inside a map: rank-0 neighbourhoods"""
    pts = np.concatenate([base, np.zeros((k + 5, 3), np.float32)])
    return pts[rng.permutation(len(pts))]


@pytest.fixture(scope="module")
def clouds():
    import rgc_slam_amd.synth as synth
    rng = np.random.default_rng(20261016)
    _, base = synth.make_world_and_map(3000, seed=synth.SEED + 31)
    base = base - base.mean(axis=0).astype(np.float32)          # (around the origin, where the invalid returns go)
    return dict(map=base, lattice=_lattice(rng), clump=_clump(rng), pole=_pole(base, rng), base=base, rng=rng)


def _check(orc, pts, k, name, tally):
    idx_r, key_r = kr.knn(pts, k)
    idx_o, d2_o = orc.knn(pts, k=k)
    bad = np.flatnonzero(np.any(idx_o != idx_r, axis=1))
    assert bad.size == 0, f"{name} k={k}: {bad.size} neighbour rows differ, first {bad[:3]}: oracle {idx_o[bad[0]]} reference {idx_r[bad[0]]}"
    assert np.array_equal(d2_o.view(np.int32), key_r.view(np.int32)), f"{name} k={k}: fp32 keys differ"
    S = kr.sample_covariances(pts, idx_r)
    e = kr.row_rel_err(orc.covariances_m(pts, orc.REG_NONE, k=k), S)
    assert e.max() <= 1e-12, f"{name} k={k}: NONE {e.max():.2e} on {np.sum(e > 1e-12)} rows"
    e = kr.row_rel_err(orc.covariances_m(pts, orc.REG_MIN_EIG, k=k), kr.regularize(S, "MIN_EIG"))
    assert e.max() <= 1e-12, f"{name} k={k}: MIN_EIG {e.max():.2e}"
    gap = kr.eigengap(S)
    ok = gap >= kr.GAP_MIN
    plane_o = orc.covariances_m(pts, orc.REG_PLANE, k=k)
    e = np.abs(plane_o - kr.regularize(S, "PLANE")).reshape(len(pts), -1).max(axis=1)
    assert e[ok].max(initial=0.0) <= 1e-9, f"{name} k={k}: PLANE {e[ok].max():.2e} on {np.sum(e[ok] > 1e-9)} rows"
    tally[name] = tally.get(name, 0) + int(np.sum(~ok))
    return idx_r, S, ok


def test_oracle_equals_the_reference_at_every_k(orc, clouds):
    tally = {}
    for k in K_ALL:
        if k == 3:
            tally = {}              # (k = 2: two points span a line, no row has a normal)
        for name in ("map", "lattice", "clump", "pole"):
            _check(orc, clouds[name], k, name, tally)
        _check(orc, _origin_copies(clouds["base"], clouds["rng"], k), k, "origin", tally)
    print("rows skipped for PLANE (eigengap below %.0e), summed over k = 3..32: %s" % (kr.GAP_MIN, tally))
    # the lattice's symmetric rows, the pole and the copies are where the normal may be undefined; on the map almost every row is compared
    assert tally["map"] < 0.01 * len(clouds["map"]) * (len(K_ALL) - 1)


@pytest.mark.parametrize("k", [2, 3, 7, 16, 19, 20, 21, 31, 32])
def test_degenerate_neighbourhoods(orc, clouds, k):
    """rank 0 (k + 5 copies of the origin) and rank 1 (the pole): the reference's covariances are exactly 0 / exactly a line, and the
    oracle's PLANE covariance there is what the Jacobi fallback makes of them -- diag(1, 1, 1e-3) for rank 0, a normal perpendicular to
    the pole for rank 1"""
    pts = _origin_copies(clouds["base"], clouds["rng"], k)
    idx, S, _ = _check(orc, pts, k, "origin", {})
    zero = np.all(pts[idx] == 0.0, axis=(1, 2))
    assert zero.sum() == k + 5                                 # every copy's k nearest are copies
    assert not S[zero].any()
    plane = orc.covariances_m(pts, orc.REG_PLANE, k=k)
    assert np.array_equal(plane[zero], np.broadcast_to(np.diag([1.0, 1.0, 1e-3]), (k + 5, 3, 3)))
    cov, nrm = orc.covariances(pts, k=k)
    assert np.array_equal(cov[zero], plane[zero])
    pts = clouds["pole"]
    idx, S, _ = _check(orc, pts, k, "pole", {})
    line = np.all((pts[idx][:, :, 0] == np.float32(2.375)) & (pts[idx][:, :, 1] == np.float32(-1.625)), axis=1)
    assert line.sum() == 60
    assert not S[line][:, :2, :].any() and np.all(S[line][:, 2, 2] > 0)
    cov, nrm = orc.covariances(pts, k=k)
    assert np.allclose(np.linalg.norm(nrm[line], axis=1), 1.0, atol=1e-12)
    assert np.abs(nrm[line][:, 2]).max() <= 1e-12                # perpendicular to the pole (z)


@pytest.mark.parametrize("extra", [0, 1])
def test_clouds_of_k_and_k_plus_one_points(orc, clouds, extra):
    """n = k: every row is the whole cloud, so all rows hold the same neighbour set; n = k + 1: each row drops exactly one point"""
    rng = np.random.default_rng(77 + extra)
    tally = {}
    for k in K_ALL:
        pts = rng.uniform(-3.0, 3.0, (k + extra, 3)).astype(np.float32)
        idx, S, _ = _check(orc, pts, k, "tiny", tally)
        if extra == 0:
            assert np.array_equal(np.sort(idx, axis=1), np.broadcast_to(np.arange(k), (k, k)))
            assert np.abs(S - S[0]).max() <= 1e-12 * np.abs(S[0]).max()
        else:
            assert len(np.unique(np.sort(idx, axis=1), axis=0)) >= 2
