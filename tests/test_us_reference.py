"""tests/us_reference.py and tests/us_cases.py held to themselves, without a GPU: every case reaches the minima of its census, the two statements of
UniformSampling agree, the two statements of the loop search agree, the vectorised travelled distance is the scalar loop's."""
import numpy as np
import pytest

import us_cases as uc
import us_reference as us

F = np.float32


def test_lattice_census_and_both_statements():
    c = uc.lattice()
    a, b = us.uniform_sampling(c, 0.5), us.uniform_sampling(c, 0.5, by_members=True)
    assert np.array_equal(a.index, b.index) and np.array_equal(a.first, b.first) and np.array_equal(a.ties, b.ties)
    assert np.array_equal(a.out.view(np.uint32), c[a.index].view(np.uint32))
    cen = a.census()
    print("lattice:", cen)
    for k, v in uc.LATTICE_MINIMA.items():
        assert cen[k] >= v, (k, cen)
    assert (c[:, :3] < 0).any() and np.array_equal(c[:, :3] * 16, np.round(c[:, :3] * 16))
    # a tie is exact: the winner is the lowest index among the members that hold the minimum
    key = us.dist2(c[:, :3], us.leaf_centres(c[:, :3], 0.5))
    for j in np.flatnonzero(a.ties)[:50]:
        mem = a.leaf.members(j)
        assert a.index[j] == mem[key[mem] == key[mem].min()].min()


@pytest.mark.parametrize("plant", ["first", "last", "boundary"])
@pytest.mark.parametrize("spread", [False, True])
def test_big_leaves_winners_are_the_planted_ones(plant, spread):
    c, planted = uc.big_leaves(plant, spread=spread)
    r = us.uniform_sampling(c, 0.5)
    pops = np.diff(r.leaf.start)
    assert set(uc.LEAF_POPULATIONS) <= set(int(x) for x in pops) and r.leaf.fullest == 6000
    assert set(int(x) for x in planted) <= set(int(x) for x in r.index)
    if plant != "last":
        assert r.ties.sum() >= len(uc.LEAF_POPULATIONS) - 3          # every leaf that has room for the copy holds an exact tie
    rank = {"first": lambda pop: 0, "last": lambda pop: pop - 1}.get(plant)
    for j in range(len(r.index)):
        mem = r.leaf.members(j)
        if len(mem) in uc.LEAF_POPULATIONS and rank is not None and r.index[j] in planted:
            assert r.index[j] == mem[rank(len(mem))]


@pytest.mark.parametrize("leaf", [0.3, 0.2])
def test_wall_points_rounding_decides(leaf):
    c = uc.walls(leaf)
    n = uc.rounding_decides(c, leaf)
    print("walls at leaf %g: the fp32 product moves %d coordinates of %d into another leaf than the exact quotient" % (leaf, n, 3 * len(c)))
    assert n >= 10 and (c[:, :3] < 0).any()
    r = us.uniform_sampling(c, leaf)
    assert len(r.index) < len(c) and (r.index != r.first).sum() >= 10


def test_unfiltered_and_empty():
    over = uc.pc.two_clusters(4000, 160.0, 31)
    r = us.uniform_sampling(over, 0.1)
    assert r.unfiltered and np.array_equal(r.index, np.arange(4000)) and np.array_equal(r.out.view(np.uint32), over.view(np.uint32))
    e = us.uniform_sampling(np.zeros((0, 4), F), 0.3)
    assert len(e.index) == 0 and e.out.shape == (0, 4)
    three = us.uniform_sampling(uc.lattice()[:, :3], 0.5)
    assert not three.out[:, 3].any()


def test_travel_against_a_scalar_loop():
    rng = np.random.default_rng(5)
    poses = np.cumsum(rng.normal(0, 0.4, (300, 6)), axis=0).astype(F)
    poses[:, 5] = ((poses[:, 5] * 3 + np.pi) % (2 * np.pi) - np.pi).astype(F)            # yaw wraps many times
    d, a = us.travel(poses)
    dd, aa = [F(0)], [F(0)]
    for p in range(1, len(poses)):
        x, y = us.travel_step(dd[-1], aa[-1], poses[p - 1], poses[p])
        dd.append(x); aa.append(y)
    assert np.array_equal(d.view(np.uint32), np.array(dd, F).view(np.uint32)) and np.array_equal(a.view(np.uint32), np.array(aa, F).view(np.uint32))
    raw = np.abs(np.diff(poses[:, 5].astype(np.float64)))
    assert (raw > np.pi).sum() >= 20, "the wrap is exercised"
    assert d[0] == 0 and a[0] == 0 and (np.diff(d) >= 0).all()


def test_gate_is_strict():
    q = np.array([1.0, -2.0, 0.5], F)
    for (dx, dy), radius in (((3.0, 4.0), 5.0), ((9.0, 12.0), 15.0)):
        on = q + np.array([dx, dy, 0.0], F)
        just_in = q + np.array([dx, np.nextafter(F(dy), F(0)), 0.0], F)
        inside, d2, r2 = us.gate(np.stack([on, just_in]), q, radius)
        assert d2[0] == r2 and list(inside) == [False, True], (d2, r2)


@pytest.mark.parametrize("n", uc.STORE_SIZES)
def test_lattice_drive_selections(n):
    poses, ids = uc.lattice_drive(n)
    g_ids, g = us.select_global(poses[:, :3], ids, 0.5)
    assert len(g_ids) == len(g.index) and set(g_ids) <= set(ids)
    centre = poses[n // 2, :3] + np.array([0.03, 0.02, 0.0], F)
    s_ids, n_in, s = us.select_surrounding(poses[:, :3], ids, centre, 3.0, 0.5)
    assert 1 <= n_in <= n and len(s_ids) >= 1
    if n == 5000:
        assert g.census()["tie_leaves"] >= 20 and s.census()["tie_leaves"] >= 20 and n_in < n and (g.index != g.first).sum() >= 100, (g.census(), s.census())
        s3, n3, u3 = us.select_surrounding(poses[:, :3], ids, centre, 3.0, 0.3)
        assert n3 == n_in and len(s3) > len(s_ids)


def _square():
    poses, ids = uc.square_drive()
    d, _ = us.travel(poses)
    return poses, ids, d, np.full(len(ids), 8)


def test_square_drive_loop_both_statements():
    poses, ids, d, nf = _square()
    a, b = us.detect_loop(poses[:, :3], ids, d, nf), us.detect_loop_literal(poses[:, :3], ids, d, nf)
    assert a == b
    L, R, inside, d2, passes = us._loop_setup(poses[:, :3], d, us.LOOP_DEFAULTS)
    qualify = int((inside & passes & (ids >= 10)).sum())
    print("square drive: R = %.4f, %d in radius, %d qualify, %d nearer poses skipped for their id, closest %d, history %d..%d"
          % (R, a["n_in_radius"], qualify, a["nearer_skipped_for_id"], a["closest_id"], a["history_ids"][0], a["history_ids"][-1]))
    assert abs(float(R) - 7.47) < 1e-5 and d[-1] == F(123.5)
    assert a["n_in_radius"] >= uc.SQUARE_MINIMA["n_in_radius"] and qualify >= uc.SQUARE_MINIMA["qualify"]
    assert a["nearer_skipped_for_id"] >= uc.SQUARE_MINIMA["nearer_skipped_for_id"]
    assert a["found"] and a["closest_id"] == 10 and a["latest_id"] == 247
    assert a["history_ids"] == list(range(0, 61))                                       # clipped at 0
    wide = us.detect_loop(poses[:, :3], ids, d, nf, history_search_num=300)
    assert wide["history_ids"] == list(range(0, 247))                                   # clipped at L
    for kw in (dict(distance_by_loop=-5000.0), dict(history_search_radius=-10.0), dict(min_key_id=0), dict(loop_keyframe_dis_diff=200.0)):
        x, y = us.detect_loop(poses[:, :3], ids, d, nf, **kw), us.detect_loop_literal(poses[:, :3], ids, d, nf, **kw)
        assert x == y, kw
    assert not us.detect_loop(poses[:, :3], ids, d, nf, distance_by_loop=-5000.0)["found"]
    neg = us.detect_loop(poses[:, :3], ids, d, nf, history_search_radius=-10.0)
    assert neg["search_radius"] < 0 and neg["found"] and neg["n_in_radius"] >= 30
    bare = us.detect_loop(poses[:, :3], ids, d, np.zeros(len(ids), int))
    assert not bare["found"] and bare["closest_id"] == 10 and len(bare["history_ids"]) == 61
    other = 3 * ids + 1
    o = us.detect_loop(poses[:, :3], other, d, nf)
    assert o == us.detect_loop_literal(poses[:, :3], other, d, nf) and o["closest_id"] == 3 * 7 + 1 and o["closest_pos"] == 7


def test_loop_statements_agree_on_random_drives():
    rng = np.random.default_rng(8)
    found = 0
    for k in range(40):
        n = int(rng.integers(1, 400))
        poses = np.zeros((n, 6), F)
        poses[:, :3] = (np.cumsum(rng.integers(-3, 4, (n, 3)), axis=0) / 2.0).astype(F)          # a lattice walk: equal distances happen
        ids = np.arange(n) if k % 2 else rng.permutation(n)
        d, _ = us.travel(poses)
        nf = rng.integers(0, 3, n)
        kw = dict(loop_keyframe_dis_diff=float(rng.choice([0.0, 5.0, 20.0])), history_search_num=int(rng.integers(0, 60)))
        a, b = us.detect_loop(poses[:, :3], ids, d, nf, **kw), us.detect_loop_literal(poses[:, :3], ids, d, nf, **kw)
        assert a == b, (k, a, b)
        found += a["found"]
    assert found >= 5
    assert not us.detect_loop(np.zeros((0, 3)), np.zeros(0, int), np.zeros(0, F), np.zeros(0, int))["found"]
