"""The DEVICE compile of the device LM's scalar code -- so3_exp_R's two series, solve_ldlt6's v_rcp_f64 and Newton steps, lm_try, lm_step_decide --
in one-lane kernels (tests/cpp/lm_device_table.hip, built here with hipcc for gfx950, run once as a child process) against the longdouble reference on
the tables of tests/lm_cases.py: the same checks as tests/test_lm_reference.py makes of the host compile, at 4 x the host's measured deviation (at
least 8 x 2^-53), lambda to 4 ulp, integers, flags and copied doubles equal, untouched fields bit for bit.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

import lm_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """both halves' result tables: one build, one child process with a time limit (read only)"""
    td = tmp_path_factory.mktemp("lm_device")
    return lc.run_harness(lc.build_harness(td / "lm_device_table", device=True), td, host_only=False)


@pytest.fixture(scope="module")
def checked(both):
    return lc.check_all(both["device"], device=True)


@pytest.mark.parametrize("table", ["exp", "solve", "tries", "decide", "scripts"])
def test_device_compile_against_the_reference(checked, table):
    fig, bad = checked[table]
    print(table, {k: round(v, 3) for k, v in fig.items()}, "(units of 2^-53; lambda in ulps)")
    assert bad == []


def test_the_host_half_of_this_build_is_the_host_build(both):
    """hipcc's host compile of the same functions passes the host's own bars too (clang for g++: the same IEEE operations, -ffp-contract=off)"""
    for table, (fig, bad) in lc.check_all(both["host"], device=False).items():
        assert bad == [], table


def test_the_tables_reach_the_devices_own_arithmetic(both):
    """the device's series is not the host's closed form, bit for bit, somewhere between its two edges -- were every row equal, the table would be
    comparing one arithmetic with itself -- and below theta^2 = 1e-10 both run the same polynomial: equal there"""
    th2 = np.array([float(c[0] @ c[0]) for c in lc.exp_cases()])
    h, d = both["host"][0]["R"], both["device"][0]["R"]
    series = (th2 >= 1.0e-9) & (th2 < 0.24)
    differ = int((h[series] != d[series]).any(axis=1).sum())
    print(f"so3_exp_R: {differ} of {int(series.sum())} rows between the edges differ from the host's by a bit or more")
    assert series.sum() >= 64 and differ >= 8
    assert np.array_equal(h[th2 < 0.9e-10], d[th2 < 0.9e-10])


def test_failed_solves_on_the_device(both):
    """the NaN pattern of a refused system, entry for entry the host's; the decisions' integers and flags equal the host's on every row"""
    h, d = both["host"], both["device"]
    for name in ("d", "delta", "xi"):
        assert np.array_equal(np.isnan(h[2][name]), np.isnan(d[2][name]))
    assert np.array_equal(h[1]["ok"], d[1]["ok"])
    for t in (3, 4):
        for n in ("inner", "outer", "done", "conv", "failed", "mode", "cur", "n_lin", "n_err", "ncorr"):
            assert np.array_equal(h[t]["st"][n], d[t]["st"][n]), (t, n)
        assert np.array_equal(h[t]["took_xi"], d[t]["took_xi"])
