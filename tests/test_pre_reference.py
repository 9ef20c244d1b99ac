"""The oracle's leaf filter, de-skew and re-framing (oracle/rgc_oracle.c) held to the independent reference of tests/pre_reference.py, on every input family
the GPU test (tests/test_gpu_pre_routes.py) uses.  No GPU.  Leaf filter: shapes equal and arrays bit-equal.  De-skew and re-framing: one fp32 ulp at the
reference's value plus the fp64 error of the terms (pre_reference.ulp_bound, derived in its docstring).  This is also where the inputs are sized: the route
rule is restated in tests/pre_cases.py and the intended route of every case is printed and checked against the table row the case is for."""
import numpy as np
import pytest

import pre_cases as pc
import pre_reference as pr


def _bit_equal(got, ref):
    return got.shape == ref.out.shape and np.array_equal(got.view(np.uint32), ref.out.view(np.uint32))


def _hold(orc, cloud, leaf, what):
    ref = pr.voxelgrid(cloud, leaf)
    got = orc.voxelgrid_filter(pr.four_columns(cloud), leaf)
    assert _bit_equal(got, ref), "%s leaf %g: %s" % (what, leaf, pr.explain_mismatch(ref, got))
    return ref


def test_reference_sum_is_the_sequential_sum():
    """the vectorised segmented sum against a python loop over the members, one leaf at a time"""
    c = pc.row_line(300, 3000, 0.2, 5)
    ref = pr.voxelgrid(c, 0.2)
    for j in list(range(0, len(ref.out), 97)) + [int(np.argmax(np.diff(ref.start)))]:
        acc = np.zeros(4, np.float32)
        mem = ref.members(j)
        assert (np.diff(mem) > 0).all()                        # ascending point index
        for i in mem:
            acc = acc + c[i]
        assert np.array_equal(ref.out[j], acc / np.float32(len(mem)))
    assert (np.diff(ref.leaf_index) > 0).all()


def test_slerp_and_rotation_against_scipy():
    sst = pytest.importorskip("scipy.spatial.transform")
    for name, q in pc.deskew_quats().items():
        if "norm" in name or "fp32" in name:
            continue                                            # scipy normalises: unit quaternions only
        s = np.linspace(0, 1, 11)
        qi = np.asarray(pr.quat_inverse(q), np.float64)
        mine = pr.slerp_from_identity(s, pr.quat_inverse(q)).astype(np.float64)
        theirs = sst.Slerp([0, 1], sst.Rotation.from_quat([[0, 0, 0, 1.0], qi]))(s)
        Rm = pr.rotation_matrix(mine).astype(np.float64)
        assert np.abs(Rm - theirs.as_matrix()).max() < 1e-13, name
    for q in pc.random_unit_quats(20, 3):
        assert np.abs(pr.rotation_matrix(q).astype(np.float64) - sst.Rotation.from_quat(q).as_matrix()).max() < 1e-15


def test_route_cases_are_sized_for_their_routes(orc, capsys):
    """every row of the route table: the oracle bit-equal to the reference at full size, and the intended route (the rule restated) is the row's"""
    lines = []
    for name, cs in pc.route_cases().items():
        for which, n in (("fresh", cs["n_fresh"]), ("kept", cs["n_kept"])):
            cloud = cs["make"](n)
            assert len(cloud) == n
            if name == "segments_1300k" and which == "kept":
                ref = pr.voxelgrid(cloud, cs["leaf"])             # (the same cloud as `fresh`: held to the oracle once)
            else:
                ref = _hold(orc, cloud, cs["leaf"], name)
            if which == "fresh":
                route = pc.intended_route(ref.div, n)
                box = ref.div
            else:
                route = pc.intended_route(box, n, kept=True)
                assert (ref.div <= box).all()
            lines.append("%-18s %-5s n=%-8d leaf=%g grid=%s fullest leaf=%d fullest row=%d -> %s %s" % (
                name, which, n, cs["leaf"], list(map(int, ref.div)), ref.fullest, pc.fullest_row(cloud, cs["leaf"]), pc.label(route), route))
            assert pc.label(route) == (cs["want"] if which == "fresh" else cs["want_kept"]), lines[-1]
            if cs.get("fullest_over"):
                assert pc.fullest_row(cloud, cs["leaf"]) > cs["fullest_over"]
                assert ref.fullest >= 4                          # several points per leaf on the line
            if cs.get("wide_x"):
                assert ref.div[0] > 8192 and route["nseg"] == 3
                ijk = pr.leaf_coords(cloud[:, :3], cs["leaf"])
                keys = {(int(a), int(b), int(c)) for a, b, c in ijk}
                pairs = sum((a + 8192, b, c) in keys for a, b, c in keys)
                segs = set(int(a - ref.minb[0]) >> 13 for a, _, _ in keys)
                assert pairs >= n // 20 and segs == {0, 1, 2}, (pairs, segs)
    for pop in (4095, 4096, 4097):
        c = pc.exact_bucket(pop)
        ref = _hold(orc, c, 0.2, "bucket of %d" % pop)
        assert pc.fullest_row(c, 0.2) == pop and pc.label(pc.intended_route(ref.div, len(c))) == "rows packed"
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_overflow_and_its_neighbours(orc):
    """dx dy dz > INT_MAX: the input, unfiltered, 4 columns (intensity 0 for a 12-byte point); just below: filtered (sparse) -- and the grid under INT_MAX
    with more than 64e6 rows that the product refuses (RGC_ERR_GRID_TOO_LARGE) is filtered by the reference and the oracle like any other"""
    leaf = 0.1
    over = pc.two_clusters(4000, 160.0, 31)                     # (160 + 40)^2 * (160 + 10) m^3 at 0.1 m: 2000 * 2000 * 1700 > INT_MAX
    ref = pr.voxelgrid(over, leaf)
    assert ref.unfiltered and np.array_equal(ref.out, over) and pc.intended_route(ref.div, len(over))["kind"] == "copy"
    assert np.array_equal(orc.voxelgrid_filter(over, leaf), over)
    r3 = pr.voxelgrid(over[:, :3], leaf)
    assert r3.unfiltered and r3.out.shape == (4000, 4) and not r3.out[:, 3].any()
    assert np.abs(over[:, :3]).max() * 10 < 1e9
    under = pc.two_clusters(4000, 60.0, 31)                     # 1000 * 1000 * 700 leaves, 7e5 rows: sparse, filtered
    ref = _hold(orc, under, leaf, "under")
    assert not ref.unfiltered and pc.intended_route(ref.div, len(under))["kind"] == "chain"
    refused = pc.two_clusters(4000, (0.0, 8050.0, 8050.0), 31, span=(20.0, 40.0, 40.0))  # 20 x 8090 x 8090 leaves of 1 m: under INT_MAX, 65e6 rows
    ref = pr.voxelgrid(refused, 1.0)
    route = pc.intended_route(ref.div, len(refused))
    assert not ref.unfiltered, ref.div
    assert route["kind"] == "refused" and float(ref.div[1]) * ref.div[2] > 64e6, (ref.div, route)
    _hold(orc, refused, 1.0, "refused by the product, filtered by PCL")


def test_leaf_sizes_walls_sizes_and_strides(orc):
    sw = pc.sweep(n_az=600)
    for leaf in pc.LEAVES_IN_USE + pc.LEAVES_BEYOND + pc.drawn_leaves():
        _hold(orc, sw, leaf, "sweep")
        _hold(orc, pc.wall_points(leaf, 41), leaf, "walls")
    for leaf in (0.05, 0.1, 0.15, 0.25):
        for far in (500.0, 1000.0):
            ref = _hold(orc, pc.wall_points(leaf, 42, far=far), leaf, "walls at %g m" % far)
            assert not ref.unfiltered
    for n in pc.SIZES:
        for kind, c in pc.sized_clouds(n, 43).items():
            ref = _hold(orc, c, 0.2, "%s n=%d" % (kind, n))
            assert len(ref.out) == {"one_leaf": 1, "own_leaf": n, "runs_of_3": (n + 2) // 3}[kind], (kind, n, len(ref.out))
    for st in pc.STRIDES:                                        # the reference's view of a strided cloud: the first 3 or 4 floats of every row
        a = pc.strided(sw, st)
        assert np.array_equal(pr.voxelgrid(a, 0.3).out, pr.voxelgrid(sw[:, :3] if st == 12 else sw, 0.3).out)


def _max_ulps(got, ref, p, t):
    bound = pr.ulp_bound(ref, np.linalg.norm(p[:, :3].astype(np.float64), axis=1), np.full(len(p), np.linalg.norm(t)))
    err = np.abs(got[:, :3].astype(np.float64) - ref).astype(np.float64)
    w, k = pr.worst_in_ulps(got[:, :3], ref)
    return bool((err <= bound).all()), w, k


def test_deskew_oracle_against_the_reference(orc, capsys):
    worst = 0.0
    for scale in (1.0, 1000.0):
        cloud = pc.deskew_cloud(scale, 51)
        for t in pc.TRANSLATIONS:
            outs = {}
            for name, q in pc.deskew_quats().items():
                got = orc.deskew(cloud, q, t)
                ref = pr.deskew(cloud, q, t)
                ok, w, k = _max_ulps(got, ref, cloud, t)
                worst = max(worst, w)
                assert ok, "deskew %s |p|~%g |t|=%.4g: %.3f ulp at point %d" % (name, scale, np.linalg.norm(t), w, k // 3)
                assert np.array_equal(got[:, 3], cloud[:, 3])
                outs[name] = got
            for name in outs:                                    # q and -q are the same rotation: the same cloud, bit for bit
                if "-(" + name + ")" in outs:
                    assert np.array_equal(outs[name], outs["-(" + name + ")"]), name
    with capsys.disabled():
        print("\nde-skew: worst %.3f ulp" % worst)


def test_transform_oracle_against_the_reference(orc, capsys):
    worst = 0.0
    rng = np.random.default_rng(61)
    quats = list(pc.deskew_quats().values()) + list(pc.random_unit_quats(12, 62))
    for scale in (1.0, 1000.0, 1.0e4):
        cloud = pc.deskew_cloud(scale, 63)
        for q in quats:
            for tn in (0.3, 300.0, 1.0e4):
                t = rng.normal(size=3); t *= tn / np.linalg.norm(t)
                got, ref = orc.transform_cloud(cloud, q, t), pr.transform(cloud, q, t)
                ok, w, k = _max_ulps(got, ref, cloud, t)
                worst = max(worst, w)
                assert ok, ("transform", scale, q, t, w, k)
                assert np.array_equal(got[:, 3], cloud[:, 3])
    with capsys.disabled():
        print("\nre-framing: worst %.3f ulp" % worst)
