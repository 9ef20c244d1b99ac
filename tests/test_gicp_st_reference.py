"""The FastGICPSingleThread reference (tests/gicp_st_reference.py) held to itself, without a GPU: its vectorised and its literal statement agree, its
first linearisation after a reset IS FastGICP's, and every designed case (tests/gicp_st_cases.py) holds what it was designed to hold -- counted by the
reference alone."""
import numpy as np
import pytest

import gicp_reference as gr
import gicp_st_cases as cases
import gicp_st_reference as sr

REL = 1e-5          # the bar tests/test_gpu_gicp_st.py compares cost, H and b at


@pytest.mark.parametrize("case", cases.designed_cases(), ids=lambda c: c["name"])
def test_designed_case_reaches_its_minima(case):
    _, total = cases.run_reference(case)
    print(case["name"], total)
    for k, v in case["minima"].items():
        assert total[k] >= v, (case["name"], k, total[k], v)


@pytest.mark.parametrize("n", cases.SIZES)
def test_sizes_steps_are_all_none_mixed_all(n):
    case = cases.sizes_case(n)
    seen = []
    cases.run_reference(case, lambda ref, T, sums: seen.append(ref.num_searched()))
    assert seen[0] == n and seen[1] == 0 and 0 < seen[2] < n and seen[3] == n, seen


def test_walls_second_nearest_is_the_one_across():
    case = cases.walls_case()
    ref, _ = cases.run_reference(case)
    k1, k2 = ref.state["key1"].astype(np.float64), ref.state["key2"].astype(np.float64)
    assert np.allclose(np.sqrt(k1), 0.05, atol=1e-4)
    want = np.repeat([0.11, 0.11 * np.sqrt(2), 0.11 * np.sqrt(3)], 4)
    assert np.allclose(np.sqrt(k2), want, atol=1e-4), np.sqrt(k2)
    assert (ref.state["searched"] == 0).all()                        # the 1 mm step skipped every one of them


def test_sticky_pairs_flip_only_after_a_reset():
    case = cases.sticky_case()
    corr = []
    cases.run_reference(case, lambda ref, T, sums: corr.append(ref.state["corr"].tolist()))
    assert corr == [[0, -1], [0, -1], [-1, 0]], corr


@pytest.mark.parametrize("name", ["sizes_65", "two_points", "duplicates", "sticky", "stale_M", "walls"])
def test_vectorised_and_literal_agree(name):
    case = next(c for c in cases.designed_cases() if c["name"] == name)
    lit = sr.Literal(case["src"], case["cov_s"], case["tgt"], case["cov_t"], case["d_max"])
    ref = cases.make_reference(case)
    for step in case["steps"]:
        if isinstance(step, str):
            ref.reset()
            lit.anchors = []
            continue
        y, H, b = ref.linearize(step)
        yl, Hl, bl = lit.linearize(step)
        st = ref.state
        assert st["corr"].tolist() == lit.corr and st["searched"].tolist() == lit.searched
        assert np.array_equal(st["key1"], np.array(lit.sq, np.float32)) and np.array_equal(st["key2"], np.array(lit.sq2, np.float32))
        assert abs(y - yl) <= 1e-9 * max(abs(yl), 1e-300)
        assert np.abs(H - Hl).max() <= 1e-9 * max(np.abs(Hl).max(), 1e-300) and np.abs(b - bl).max() <= 1e-9 * max(np.abs(bl).max(), 1e-300)
        T3 = cases.translation(0.01, -0.02, 0.005) @ step
        e, el = ref.compute_error(T3), lit.compute_error(T3)
        assert abs(e - el) <= 1e-9 * max(abs(el), 1e-300)


@pytest.mark.parametrize("name", ["sizes_257", "lattice_ties", "outside"])
def test_first_linearisation_is_fastgicp(name):
    case = next(c for c in cases.designed_cases() if c["name"] == name)
    ref = cases.make_reference(case)
    plain = gr.GICP(case["d_max"])
    plain.set_target(case["tgt"], case["cov_t"])
    plain.set_source(case["src"], case["cov_s"])
    for T in [s for s in case["steps"] if not isinstance(s, str)]:
        ref.reset()
        y, H, b = ref.linearize(T)
        yp, Hp, bp = plain.linearize(T)
        assert y == yp and np.array_equal(H, Hp) and np.array_equal(b, bp)
        assert np.array_equal(ref.state["corr"], plain.corr[0]) and np.array_equal(ref.state["key1"], plain.corr[1])
        assert ref.num_searched() == len(case["src"])


def test_stale_M_differs_from_fastgicp_by_far_more_than_the_bar():
    """at the second pose of stale_M every point is skipped: the cost under the kept matrices differs from FastGICP's cost at the same pose (the
    same pairs, M recomputed) by at least 100 x the comparison bar -- a product that recomputed M would not pass the GPU comparison"""
    case = cases.stale_case()
    ref, total = cases.run_reference(case)
    T = case["steps"][-1]
    assert ref.num_searched() == 0 and total["stale"] == len(case["src"])
    plain = gr.GICP(case["d_max"])
    plain.set_target(case["tgt"], case["cov_t"])
    plain.set_source(case["src"], case["cov_s"])
    yp, Hp, bp = plain.linearize(T)
    y, H, b = ref.sums(T)
    assert np.array_equal(plain.corr[0], ref.state["corr"])
    rel = abs(y - yp) / abs(yp)
    print("stale_M: single-thread cost %.6g, FastGICP cost %.6g at the same pose: relative difference %.3g (bar %.1g)" % (y, yp, rel, REL))
    assert rel >= 100 * REL
    assert np.abs(H - Hp).max() / np.abs(Hp).max() >= 100 * REL


def test_one_point_target_never_searches_again():
    rng = np.random.default_rng(5)
    src = rng.uniform(-1, 1, (20, 3)).astype(np.float32)
    ref = sr.GICPST()
    ref.set_target(np.zeros((1, 3), np.float32), np.eye(3)[None])
    ref.set_source(src, np.broadcast_to(np.eye(3), (20, 3, 3)))
    ref.linearize(np.eye(4))
    assert np.isinf(ref.state["key2"]).all()
    ref.linearize(cases.translation(5.0))
    assert ref.num_searched() == 0
