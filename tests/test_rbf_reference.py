"""tests/rbf_reference.py against itself and against what can be known without it (no GPU): the query-centred moments and the literal restatement of
covariance_estimation_rbf.cu agree within the bar the GPU is held to; the dyadic lattice has the ball arithmetic says it has; the knife-edge pairs are
members; the gap rule leaves out at most 5 % of any case's rows."""
import numpy as np
import pytest

import rbf_cases as rc
import rbf_reference as rr


@pytest.mark.parametrize("name", rc.NONE_CASES)
def test_shifted_and_literal_forms_agree(name):
    """The literal form sums around the origin: its own longdouble error is 2^-64 m |p|^2 per entry, which is added to the bar (it is nothing of the
    product's: at the scene's coordinates, 450 m, that is 1e-12; the query-centred form's is below 1e-17)."""
    P, kw, md, _ = rc.case(name)
    m = rc.mom(name)
    lit = rr.literal(P, kw, md)
    B = rr.bound_none(m)
    own = (m["m"] + 8)[:, None, None] * 2.0 ** -63 * (np.abs(P.astype(np.float64)) ** 2).sum(axis=1).max() * 4
    assert np.all(np.abs(lit - m["cov"]) <= B + own), float(np.max(np.abs(lit - m["cov"]) - B - own))


@pytest.mark.parametrize("res", ["0.5", "1", "2"])
def test_lattice_ball(res):
    P, kw, md, _ = rc.case("lattice_" + res)
    m = rc.mom("lattice_" + res)
    inside = rc.lattice_interior(P)
    assert inside.sum() == 9 ** 3
    assert np.all(m["m"][inside] == 257) and np.all(m["on_radius"][inside] == 6)
    assert m["m"].min() < 257


def test_knife_edge_pairs_are_members():
    P, kw, md, _ = rc.case("knife")
    _, B = rr.balls(P, md)
    for a, b in ((0, 1), (2, 3)):
        assert float(P[b, 0]) - float(P[a, 0]) > 3.0                     # farther than max_dist in exact arithmetic
        ia, ka = B[a]
        assert b in ia and ka[list(ia).index(b)] == np.float32(9.0)
        assert a in B[b][0]
    # ... at a cell offset of 4 on the grid's own walls: floor(x / res - 0.5)
    assert int(np.floor(float(P[3, 0]) - 0.5)) - int(np.floor(float(P[2, 0]) - 0.5)) == 4


@pytest.mark.parametrize("name", rc.EIGEN_CASES)
@pytest.mark.parametrize("method", ["MIN_EIG", "NORMALIZED_MIN_EIG", "PLANE"])
def test_gap_rule_leaves_out_at_most_five_percent(name, method):
    _, ok = rr.bound(rc.mom(name), method)
    assert (~ok).mean() <= 0.05, (~ok).mean()


def test_isolated_point_and_regularisations():
    m = rc.mom("isolated")
    i = rc.ISOLATED_ROW
    assert m["m"][i] == 1 and m["S0"][i] == 1.0 and np.all(m["cov"][i] == 0)
    Z = m["cov"][i:i + 1]
    assert np.all(rr.regularize(Z, "NONE") == 0)
    assert np.allclose(rr.regularize(Z, "MIN_EIG")[0], 1e-3 * np.eye(3), rtol=0, atol=1e-18)
    assert np.allclose(rr.regularize(Z, "NORMALIZED_MIN_EIG")[0], 1e-3 * np.eye(3), rtol=0, atol=1e-18)
    assert np.allclose(np.linalg.eigvalsh(rr.regularize(Z, "PLANE")[0]), [1e-3, 1, 1], rtol=0, atol=1e-15)
    assert np.allclose(rr.regularize(Z, "FROBENIUS")[0], np.sqrt(3.0) * np.eye(3), rtol=1e-14, atol=0)


def test_defaults_of_max_dist():
    assert rr.effective_max_dist(0.5, -1.0) == 2.5 and rr.effective_max_dist(0.5, 0.0) == 2.5 and rr.effective_max_dist(0.5, 3.0) == 3.0
