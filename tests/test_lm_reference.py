"""No GPU: the HOST compile of the device LM's scalar code (csrc/rgc_lm.h, csrc/rgc_lm_decide.h; built by g++ into tests/cpp/lm_device_table.hip's
host half, run once as a child process) against the longdouble reference (tests/lm_reference.py) on every designed case (tests/lm_cases.py): so3_exp_R,
solve_ldlt6, lm_try, every branch of lm_step_decide on injected states, and the scripted solves.  The host's deviations measured here are the figures
the device's bars are made of (lm_cases.HOST_FIGURES: the device gets 4 x, at least 8 x 2^-53, in tests/test_gpu_lm_scalar.py); the host is held to the
figures themselves, so they cannot go stale.  Also: the reference against independent formulas, and what the designed cases reach.

Planted errors, each shown once to fail here (a scratch copy of csrc's headers with the one change, `python tests/lm_cases.py --csrc <copy>`, at the
host's bars and again at the device's with --device-bars; nothing of it is committed).  Violations per table (exp, solve, tries, decide, scripts):
    rho <= 0 for rho < 0 (lm_step_decide)                               decide 1651
    m <= 1 for m < 1 (lm_is_converged)                                  decide 4776
    nu not reset at the end of an outer iteration                       decide 1560, scripts 3
    fmin for fmax in the lambda factor                                  decide 1040, scripts 14
    inner > max_inner for inner >= max_inner                            decide 858, scripts 7
    LDL^T: D[j] skipped in one update (j = 2 of row 4's)                solve 55, tries 105, decide 2184, scripts 24
  with the device guard of so3_exp_R's series lifted in the scratch copy (the host then runs the series; unmutated it passes at the device's bars):
    the sign of the 1/5040 term flipped                                 exp 160, tries 126   (device bars)
    the 1/39916800 term dropped                                         exp 64, tries 27     (device bars; only theta within 1e-3 of 0.5 sees it)
    the 1/3628800 term dropped                                          exp 112, tries 72    (device bars)"""
import numpy as np
import pytest

import lm_cases as lc
import lm_reference as ref


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the host half's five result tables (one build, one child process; read only)"""
    td = tmp_path_factory.mktemp("lm_host")
    return lc.run_harness(lc.build_harness(td / "lm_device_table", device=False), td, host_only=True)["host"]


@pytest.fixture(scope="module")
def checked(host):
    return lc.check_all(host, device=False)


@pytest.mark.parametrize("table", ["exp", "solve", "tries", "decide", "scripts"])
def test_host_compile_against_the_reference(checked, table):
    fig, bad = checked[table]
    print(table, {k: round(v, 3) for k, v in fig.items()}, "(units of 2^-53; lambda in ulps)")
    assert bad == []
    for k, v in fig.items():
        if k in lc.HOST_FIGURES:
            assert v <= lc.HOST_FIGURES[k], (k, v)
            if table in ("exp", "solve"):
                assert v >= 0.5 * lc.HOST_FIGURES[k], f"{k}: the recorded figure {lc.HOST_FIGURES[k]} is stale, the host is at {v:.3f}"


def test_recorded_figures_are_the_hosts(checked):
    """try_R and try_xi are taken over the three tables that make tries; the recorded figure is within a factor two of the largest"""
    for k in ("try_R", "try_xi"):
        m = max(checked[t][0].get(k, 0.0) for t in ("tries", "decide", "scripts"))
        assert 0.5 * lc.HOST_FIGURES[k] <= m <= lc.HOST_FIGURES[k], (k, m)
    assert lc.bar("solve_bwd", True) == 8.0 and lc.bar("exp_R_large", True) == 4 * lc.HOST_FIGURES["exp_R_large"]


def test_reference_rotation_is_rodrigues():
    """the quaternion route against I + sin(th) K + (1 - cos(th)) K^2 in longdouble, and R^T R = I, over the table's own inputs"""
    worst = 0.0
    for w, _, _, _ in lc.exp_cases()[::3]:
        R = ref.so3_exp_R(w)
        wl = ref.ld(w)
        th = np.sqrt(wl @ wl)
        K = np.array([[0, -wl[2], wl[1]], [wl[2], 0, -wl[0]], [-wl[1], wl[0], 0]], dtype=ref.LD)
        if th > 1e-3:
            Rr = np.eye(3, dtype=ref.LD) + np.sin(th) / th * K + (1 - np.cos(th)) / (th * th) * (K @ K)
        else:
            Rr = np.eye(3, dtype=ref.LD) + K + (K @ K) / 2
        tol = 2.0 ** -60 if th > 1e-3 else float(th ** 3)
        worst = max(worst, float(np.abs(R - Rr).max()))
        assert float(np.abs(R - Rr).max()) <= max(tol, 2.0 ** -60) and float(np.abs(R.T @ R - np.eye(3)).max()) <= 2.0 ** -60
    print("reference rotation against Rodrigues:", worst)


def test_reference_solve():
    """the pivoted elimination: residual at longdouble precision on every accepted system, None for the zero matrix, and -- unlike the
    unpivoted device solve -- an answer for the zero fourth pivot, which is why `refused` is declared by the case and not taken from here"""
    for c in lc.solve_cases():
        A = lc._A_of(c)
        x = ref.solve6(A, -c["b"])
        if c["name"] == "e_zero":
            assert x is None
        elif not c["refused"]:
            assert ref.backward_error(A, x, -c["b"]) <= 2.0 ** -60, c["name"]
    assert [c["name"] for c in lc.solve_cases() if c["refused"]] == ["e_zero", "f_1e301", "g_pivot3"]
    conds = [np.linalg.cond(lc._A_of(c)) for c in lc.solve_cases() if not c["refused"]]
    assert min(conds) < 1.01 and max(conds) > 1e14 and sum(1 for k in conds if k <= 1e8) >= 20


def test_convergence_threshold():
    for name, D, conv in lc._delta_variants():
        assert ref.is_converged(D, lc.ROT_EPS, lc.TRANS_EPS) == conv, name
    assert len(lc._delta_variants()) == 26


def test_failed_solve_is_nan_entry_for_entry(host):
    """H = 0, lambda = 0: every d, the rotation and translation of delta and the first three rows of xi NaN; the last row of delta is
    (0, 0, 0, 1), so the last row of xi is x0's -- in the reference and in the host compile"""
    cases = lc.try_cases()
    rows = [i for i, c in enumerate(cases) if c["refused"]]
    assert len(rows) == 9
    for i in rows:
        assert np.isnan(host[2]["d"][i]).all() and np.isnan(host[2]["delta"][i][:12]).all() and np.isnan(host[2]["xi"][i][:12]).all()
        assert np.array_equal(host[2]["xi"][i][12:], cases[i]["x0"][3])


def test_what_the_decision_table_reaches():
    """every verdict of the reference's loop in both modes that try, at the first and the last inner and outer count; NaN rho accepts"""
    rows, names = lc.decide_cases()
    assert len(rows) == 4 * 9 * 26 * 2 * 2
    seen = {}
    for i in range(0, len(rows)):
        st = lc.state_dict(rows["st"][i])
        mode = int(rows["mode"][i])
        if mode == ref.MODE_LIN:
            continue
        yi = rows["folded"][i][29]
        v = ref.step_lm_try(st["x0"], st["lambda"], st["nu"], st["inner"], st["H"], st["b"], st["y0"], st["d"], st["delta"], st["xi"], yi, st["rot_eps"],
                            st["trans_eps"], st["max_inner"])[0]
        seen[(mode, v)] = seen.get((mode, v), 0) + 1
        if "rho=nan" in names[i] or "rho=+0" in names[i] or "rho=+inf" in names[i]:
            assert v == ref.ACCEPT, names[i]
        if "rho=-tiny" in names[i] or "rho=-inf" in names[i]:
            assert v != ref.ACCEPT, names[i]
    print(seen)
    assert all(seen.get((m, v), 0) >= 26 for m in (ref.MODE_BA, ref.MODE_B) for v in (ref.ACCEPT, ref.REJECT, ref.END_OUTER, ref.NOT_CONVERGED))


def test_what_the_scripts_reach():
    info = {s["name"]: s for s in lc.script_cases()[1]}
    L, BA, B = ref.MODE_LIN, ref.MODE_BA, ref.MODE_B
    assert info["three_rejections_then_accept"]["modes"] == [L, BA, B, B, B, L, BA]
    assert info["accept_accept_converge"]["modes"] == [L, BA, BA, BA] and info["accept_accept_converge"]["ref"]["conv"] == 1
    r = info["rejections_to_max_inner"]["ref"]
    assert r["failed"] == 1 and r["outer"] == 0 and r["n_err"] == 4 and info["rejections_to_max_inner"]["modes"] == [L, BA, B, B, B]
    assert info["negative_rho_converged_delta"]["trace"] == [(ref.END_OUTER, True)] and info["negative_rho_converged_delta"]["ref"]["conv"] == 1
    assert np.array_equal(info["negative_rho_converged_delta"]["ref"]["x0"], ref.ld(info["negative_rho_converged_delta"]["x0"]))
    for name, modes in (("outer_cap_in_BA", [L, BA, BA]), ("outer_cap_in_B", [L, BA, BA, B]), ("max_outer_1", [L, BA])):
        r = info[name]["ref"]
        assert info[name]["modes"] == modes and r["conv"] == 0 and r["failed"] == 0 and r["outer"] == lc.SCRIPTS[name]["max_outer"], name
