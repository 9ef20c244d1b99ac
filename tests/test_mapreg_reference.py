"""No GPU: the longdouble reference of the mapping solve (tests/mapreg_reference.py) against its own central differences and against
oracle/py_mapreg.py; the C oracle's exported orc_mapreg_evaluate against the reference, term by term, on every designed case
(tests/mapreg_cases.py); the minima every case declares; that the planted errors the GPU test must catch are visible at 100 x its bar; and the
LM paths, which the reference's restatement of the loop and the C oracle must both take."""
import numpy as np
import pytest

import mapreg_cases as mc
import mapreg_reference as ref

CASES = list(mc.SPECS)


@pytest.fixture(scope="module")
def solved():
    """per case: the oracle's factors at x0, the reference there and at x_eval (computed once, read only)"""
    out = {}
    for name in CASES:
        c = mc.build(name)
        fac = mc.associate(c, c["x0"])
        out[name] = dict(case=c, fac=fac, e0=ref.evaluate(mc.problem(c, fac), c["x0"]), e1=ref.evaluate(mc.problem(c, fac), c["x_eval"]))
    return out


@pytest.mark.parametrize("name", ["huber", "ground_pm_mp", "imu_0.004", "ground_imu"])
def test_analytic_jacobians_match_central_differences(solved, name):
    """longdouble central differences of the residuals (step 1e-7: truncation ~1e-14 |J'''|, rounding 1e-19 / 1e-7) against the analytic Jacobians"""
    c, fac = solved[name]["case"], solved[name]["fac"]
    x = ref._ld(c["x0"])
    sets, ground, imu = ref.central_differences(mc.problem(c, fac), x)
    for s in range(4):
        b = s // 2
        f = ref.edge_terms if s % 2 == 0 else ref.plane_terms
        J = f(c["feat"][s], fac[s], x[7 * b: 7 * b + 4], x[7 * b + 4: 7 * b + 7])[1]
        assert len(J) > 40 and float(np.abs(J - sets[s]).max()) <= 1e-10 * float(np.abs(J).max())
    for b in range(2):
        if c["ground"][b] is not None:
            J = ref.ground_terms(c["ground"][b], x[7 * b: 7 * b + 4], x[7 * b + 4: 7 * b + 7])[1]
            assert float(np.abs(J - ground[b]).max()) <= 1e-10 * float(np.abs(J).max()) and np.abs(J).max() > 1
    if c["imu"] is not None:
        J = ref.imu_terms(c["imu"], x[0:4], x[7:11])[1]
        assert float(np.abs(J - imu).max()) <= 1e-10 * float(np.abs(J).max()) and np.abs(J[:, 0:3]).max() > 1 and np.abs(J[:, 6:9]).max() > 1
        assert np.all(J[:, 3:6] == 0) and np.all(J[:, 9:12] == 0)


def test_pitch_clamp():
    """Quaternion2EulerAngle: |sinp| >= 1 gives +-pi/2, a constant (derivative 0); just inside, asin and its derivative"""
    h = np.sqrt(ref.LD(1) / 2)
    for sgn in (1, -1):
        q = np.array([0, sgn * h * (1 + ref.LD(1e-12)), 0, h * (1 + ref.LD(1e-12))], dtype=ref.LD)     # sinp = 2 w y just beyond +-1
        p, r, D, clamped = ref.pitch_roll(q)
        assert clamped and p == sgn * np.arccos(ref.LD(0)) and np.all(D[0] == 0)
    p, r, D, clamped = ref.pitch_roll(mc.quat([0.0, 0.7, 0.0]))
    assert not clamped and abs(float(p) - 0.7) < 1e-15 and abs(float(D[0, 1]) - 2.0) < 1e-12      # d is half the rotation vector


@pytest.mark.parametrize("name", ["smallest", "n255", "ground_pp_mm", "imu_0.4"])
def test_reference_vs_py_mapreg(solved, name):
    """the second restatement (numpy fp64, finite-difference Jacobians): residuals, cost, blocks, and its LM loop against the reference's"""
    from oracle import py_mapreg as pm
    c, fac = solved[name]["case"], solved[name]["fac"]
    x, kinds = c["x0"], ("edge", "plane", "edge", "plane")
    fd = [mc.factor_dict(fac[s], kinds[s]) for s in range(4)]
    cost = 0.0
    for b in range(2):
        q, t = x[7 * b: 7 * b + 4], x[7 * b + 4: 7 * b + 7]
        e, p = pm.residual_blocks(c["feat"][2 * b], fd[2 * b], c["feat"][2 * b + 1], fd[2 * b + 1], q, t)
        re = ref.edge_terms(c["feat"][2 * b], fac[2 * b], q, t)[0]
        rp = ref.plane_terms(c["feat"][2 * b + 1], fac[2 * b + 1], q, t)[0]
        assert e.shape == re.shape and p.shape == rp.shape
        assert (not e.size or np.abs(e - re.astype(float)).max() < 1e-13) and (not p.size or np.abs(p - rp.astype(float)).max() < 1e-13)
        cost += pm.robust_cost([e, p])
        if c["ground"][b] is not None:
            rg = pm.ground_residual(c["ground"][b], q, t)
            assert np.abs(rg - ref.ground_terms(c["ground"][b], q, t)[0].astype(float)).max() < 1e-9 * np.abs(rg).max()
            cost += 0.5 * float(rg @ rg)
    if c["imu"] is not None:
        ri = pm.imu_residual(c["imu"], x[0:4], x[7:11])
        assert np.abs(ri - ref.imu_terms(c["imu"], x[0:4], x[7:11])[0].astype(float)).max() < 1e-12 * max(1.0, np.abs(ri).max())
        cost += 0.5 * float(ri @ ri)
    assert abs(cost - float(solved[name]["e0"]["cost"])) <= 1e-12 * cost
    sets = [(c["feat"][2 * b], fd[2 * b], c["feat"][2 * b + 1], fd[2 * b + 1], c["ground"][b]) for b in range(2)]
    xp, tp = pm.lm_solve(sets, x, imu=c["imu"])
    xr, tr = ref.lm_solve(mc.problem(c, fac), x)
    assert (tp["iterations"], tp["successful"]) == (tr["iterations"], tr["successful"]) and tr["successful"] > 0
    assert np.abs(xp - xr).max() < 1e-7 and abs(tp["final_cost"] - tr["final_cost"]) <= 1e-9 * tr["final_cost"]


def test_oracle_evaluate_vs_reference(solved):
    """orc_mapreg_evaluate, entry by entry in the unit |difference| / sum |terms|, at x0 and at x_eval with the factors frozen: this measurement
    IS the bar of tests/test_gpu_mapreg_terms.py (8 x), so the constants in mapreg_cases.py must stay what is measured here"""
    worst = {False: 0.0, True: 0.0}
    for name in CASES:
        c, fac = solved[name]["case"], solved[name]["fac"]
        blocks = mc.bar_of(c) == mc.BAR
        for x, e in ((c["x0"], solved[name]["e0"]), (c["x_eval"], solved[name]["e1"])):
            H, g, cost = mc.oracle_evaluate(c, fac, x)
            dev, zeros_ok = ref.deviation(e, H, g, cost)
            print(f"{name}: oracle vs reference {dev:.3e}")
            assert zeros_ok and np.array_equal(H, H.T)
            worst[blocks] = max(worst[blocks], dev)
    print(f"largest deviation: features only {worst[False]:.3e}, with a ground or IMU block {worst[True]:.3e}")
    assert worst[False] <= mc.DEV_FEATURES <= 1.1 * worst[False] and worst[True] <= mc.DEV_ALL <= 1.1 * worst[True]
    assert mc.BAR == 8 * mc.DEV_ALL and mc.BAR_FEATURES == 8 * mc.DEV_FEATURES


def test_edge_endpoint_swap(solved):
    """point_a <-> point_b (the eigenvector's free sign): r and every J row change sign together, so H, g and the cost are unchanged"""
    c, fac = solved["huber"]["case"], solved["huber"]["fac"]
    sw = [f.copy() for f in fac]
    for s in (0, 2):
        sw[s][::2, 0:3], sw[s][::2, 3:6] = fac[s][::2, 3:6], fac[s][::2, 0:3]
    e, e0 = ref.evaluate(mc.problem(c, sw), c["x0"]), solved["huber"]["e0"]
    assert ref.deviation(e0, e["H"], e["g"], e["cost"])[0] < 1e-18
    H, g, cost = mc.oracle_evaluate(c, sw, c["x0"])
    assert ref.deviation(e0, H, g, cost)[0] <= mc.DEV_FEATURES


@pytest.mark.parametrize("name", CASES)
def test_declared_minima(solved, name):
    c, fac, m = solved[name]["case"], solved[name]["fac"], solved[name]["case"]["minima"]
    cen = mc.census(c, fac, c["x0"])
    print(name, cen)
    if "blocks" in m:
        assert cen["blocks"] == m["blocks"]
    if "total_cur" in m:
        assert cen["n_feat"][0] + cen["n_feat"][1] == m["total_cur"]
    if m.get("edge_plane_split_inside_wave"):
        assert cen["n_feat"][0] % 64 != 0
    for s in range(4):
        st = cen["sets"][s]
        if "inside" in m:
            assert st["inside"] >= m["inside"] and st["outside"] >= m["outside"]
        if "near_radius" in m:
            assert st["just_inside"] >= m["near_radius"] and st["just_outside"] >= m["near_radius"]
        if "zero_weight" in m:
            assert st["zero_weight"] >= m["zero_weight"]
        if m.get("no_factors"):
            assert st["factors"] == 0 and cen["n_feat"][s] > 0
    if "inside" in m:      # the weights vary per feature
        assert all(len(np.unique(f[:, 3])) > len(f) // 2 for f in c["feat"])
    if "ground_signs" in m:
        assert cen["ground_signs"] == m["ground_signs"] and cen["ground_margin"] > 1e-3
        assert mc.census(c, fac, c["x_eval"])["ground_signs"] == m["ground_signs"]
    if m.get("imu"):
        assert c["imu"] is not None
    if m.get("planes_ez"):
        e = solved[name]["e0"]
        assert cen["sets"][0]["factors"] == 0 and cen["sets"][2]["factors"] == 0 and cen["sets"][1]["factors"] >= 100 and cen["sets"][3]["factors"] >= 100
        # the plane fit (QR) of an exactly horizontal lattice leaves 1e-15 in n_x, n_y: with the normals set to e_z by hand the rows and columns
        # of x, y and yaw are exactly zero, in the reference and in the C oracle; with the associated ones they are 1e-15 of the diagonal
        for s in (1, 3):
            v = fac[s][:, 7] != 0
            assert np.abs(fac[s][v, 0:2]).max() < 1e-14 and np.abs(fac[s][v, 2] - 1).max() < 1e-14
        ez = [f.copy() for f in fac]
        for s in (1, 3):
            ez[s][ez[s][:, 7] != 0, 0:3] = [0.0, 0.0, 1.0]
        ee = ref.evaluate(mc.problem(c, ez), c["x0"])
        H, g, _ = mc.oracle_evaluate(c, ez, c["x0"])
        for a in (2, 3, 4, 8, 9, 10):      # yaw, x, y of either pose: unobservable, exactly
            assert np.all(ee["H"][a] == 0) and np.all(ee["H"][:, a] == 0) and ee["g"][a] == 0 and np.all(H[a] == 0) and np.all(H[:, a] == 0) and g[a] == 0
            assert np.abs(e["H"][a]).max() < 1e-12 * e["H"].max()
        assert all(e["H"][a, a] > 1 for a in (0, 1, 5, 6, 7, 11))


@pytest.mark.parametrize("name", CASES)
def test_planted_errors_show_at_100_bars(solved, name):
    """one factor dropped, rho' = 1 on one outer factor, one Jacobian column of one factor negated, the edges' 0.2 m baseline used as 0.1: each
    moves some entry of (H, g, cost) by at least 100 x the bar the GPU read-out is held to in this case"""
    c, fac, e0 = solved[name]["case"], solved[name]["fac"], solved[name]["e0"]
    need, prob, applied = 100 * mc.bar_of(c), mc.problem(c, fac), 0
    for s in range(4):
        st = e0["sets"][s]
        live = np.nonzero((st["var"] != 0) & (st["s2"] > 0))[0]
        if not len(live):
            continue
        i = int(live[np.argmin(st["s2"][live])])          # the factor that matters least
        plants = [("drop", s, i)]
        if st["outer"].any():
            plants.append(("rho1", s, int(np.nonzero(st["outer"])[0][np.argmin(st["s2"][st["outer"]])])))
        if s % 2 == 0:
            plants.append(("baseline", s))
        # (the column in which that factor's Jacobian is largest: a vertical pole's edge factor has no z column to negate)
        negcol = [ref.deviation(e0, *[ref.evaluate(prob, c["x0"], plant=("negcol", s, i, col))[k] for k in ("H", "g", "cost")])[0] for col in range(6)]
        print(name, "negcol", s, i, f"{max(negcol):.3e}")
        assert max(negcol) >= need
        for plant in plants:
            e = ref.evaluate(prob, c["x0"], plant=plant)
            moved = ref.deviation(e0, e["H"], e["g"], e["cost"])[0]
            print(name, plant, f"{moved:.3e}")
            assert moved >= need, (plant, moved, need)
            applied += 1
    assert applied > 0 or c["minima"].get("no_factors")


def _two_pass(case):
    """the reference's restatement through the two passes (association by the oracle at the restatement's own poses)"""
    x, infos = case["x0"].copy(), []
    for _ in range(2):
        x, info = ref.lm_solve(mc.problem(case, mc.associate(case, x)), x)
        infos.append(info)
    for b in range(2):
        x[7 * b: 7 * b + 4] /= np.linalg.norm(x[7 * b: 7 * b + 4])
    return x, infos


@pytest.mark.parametrize("name", mc.LM_CASES)
def test_lm_restatement_vs_oracle(name):
    """the reference's LM loop and the C oracle's: the same iterations and accepted steps in both passes, the same costs and poses; the declared
    path is the one taken; and an independent association (py_mapreg: cKDTree, eigh, lstsq) decides every feature as the oracle does at x0"""
    from oracle import py_mapreg as pm
    c = mc.build(name)
    xo, rc, tr = mc.oracle_optimize(c)
    x, infos = _two_pass(c)
    assert rc == 0
    for i in range(2):
        print(name, i, tr[i]["iterations"], tr[i]["successful"], infos[i]["stop"], [(round(s["rho"], 4), s["accepted"]) for s in infos[i]["steps"]])
        assert (tr[i]["iterations"], tr[i]["successful"]) == (infos[i]["iterations"], infos[i]["successful"])
        assert abs(tr[i]["final_cost"] - infos[i]["final_cost"]) <= 1e-12 * max(tr[i]["final_cost"], 1e-300)
    assert np.abs(x - xo).max() < 1e-12
    if name in mc.PATHS:
        for i, (stop, rejected_then_accepted) in enumerate(mc.PATHS[name]):
            acc = [s["accepted"] for s in infos[i]["steps"]]
            assert infos[i]["stop"] == stop
            if rejected_then_accepted:
                assert tr[i]["iterations"] > tr[i]["successful"] > 0 and any(not a and any(acc[k + 1:]) for k, a in enumerate(acc))
            if stop == "function":
                assert infos[i]["successful"] > 0
                if name == "lm_function":
                    assert infos[i]["iterations"] < 6 and tr[i]["iterations"] < 6          # before the cap
                if name == "lm_function_at_6" and i == 0:
                    assert infos[i]["iterations"] == 6 and tr[i]["iterations"] == 6        # the tolerance is met by the sixth step
            if stop == "cap":
                assert infos[i]["iterations"] == 6
            if stop == "gradient":
                assert infos[i]["iterations"] == 0
    for s in range(4):
        b = s // 2
        if len(c["feat"][s]):
            a = pm.associate(c["feat"][s], c["x0"][7 * b: 7 * b + 4], c["x0"][7 * b + 4: 7 * b + 7], c["corner_map"] if s % 2 == 0 else c["surf_map"],
                             "edge" if s % 2 == 0 else "plane")
            assert np.array_equal(a["valid"], mc.associate(c, c["x0"])[s][:, 7] != 0)


def test_every_path_is_built_or_named():
    taken = {stop for p in mc.PATHS.values() for stop, _ in p} | {"rejected" for p in mc.PATHS.values() if any(r for _, r in p)}
    assert taken == {"rejected", "function", "cap", "gradient"} and mc.PATHS_NOT_BUILT == ["parameter"]
    assert set(mc.PATHS) <= set(mc.LM_CASES)


def test_all_invalid_case(solved):
    """no factor at all: H = 0, g = 0, cost = 0 exactly, the loop stops at iteration 0 on the gradient, and the poses come back normalised"""
    c, e = solved["all_invalid"]["case"], solved["all_invalid"]["e0"]
    H, g, cost = mc.oracle_evaluate(c, solved["all_invalid"]["fac"], c["x0"])
    assert not H.any() and not g.any() and cost == 0 and not e["H"].any() and not e["g"].any() and e["cost"] == 0
    xo, rc, tr = mc.oracle_optimize(c)
    assert abs(np.linalg.norm(c["x0"][0:4]) - 1.5) < 1e-12 and abs(np.linalg.norm(c["x0"][7:11]) - 0.5) < 1e-12
    assert all(t["iterations"] == 0 and t["successful"] == 0 for t in tr)
    assert np.abs(xo[0:4] - c["x0"][0:4] / 1.5).max() < 1e-15 and np.abs(xo[7:11] - c["x0"][7:11] / 0.5).max() < 1e-15
    assert np.array_equal(xo[4:7], c["x0"][4:7]) and np.array_equal(xo[11:14], c["x0"][11:14])
