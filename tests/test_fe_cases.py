"""The designed front-end sweeps (tests/fe_cases.py) on the CPU: on every case the C oracle equals the literal Python restatement bit
for bit (the keys tests/fuzz/fuzz_oracle_pin_frontend.py compares -- that pin draws from the same generator as the GPU tests and has
their blind spots), and the census of tests/fe_reference.py -- counted from the restatement alone -- reaches every minimum the case
declares: the proof that the reference takes the branch the case is named for.  No GPU."""
import time

import numpy as np
import pytest

import fe_cases
import fe_reference

EXACT = ("max_ring", "max_sector", "n_cloud")   # declared as the value itself, not as a lower bound


@pytest.mark.parametrize("name", list(fe_cases.CASES))
def test_case_reaches_its_branch_and_pins_the_oracle(name, orc):
    case = fe_cases.CASES[name]
    t0 = time.process_time()            # this process's CPU time: what the case costs, whatever else the machine is doing
    raw, prm, branch = fe_cases.get(name)
    c, r = fe_reference.census(name)
    o = orc.frontend(raw, **prm)
    cpu = time.process_time() - t0
    print(name, "--", branch, "--", {k: c.get(k, 0) for k in case.minima})
    assert case.minima, "a case declares what it exists for"
    for k, v in case.minima.items():
        got = c.get(k, 0)
        assert (got == v) if k in EXACT else (got >= v), (name, k, got, v)
    if r is None:
        assert o["n_cloud"] == 0
    else:
        assert fe_reference.pin(o, r) == []
    assert case.refused == (c.get("max_sector", 0) > fe_cases.SEC_MAX)
    assert cpu < 10.0, cpu


def test_case_table():
    """the staging table is consistent with the cases built around it, every family is present, the speculative sequence names cases"""
    assert {c.family for c in fe_cases.CASES.values()} == {"near", "ties", "thresholds", "quota", "redo", "rings", "counts", "spec"}
    for (top, group), nxt in zip(fe_cases.STAGING, fe_cases.STAGING[1:] + ((None, 0),)):
        assert "ring_%d" % top in fe_cases.CASES and fe_cases.staging_group(top) == group and fe_cases.staging_group(top + 1) == nxt[1]
    assert fe_cases.RING_REFUSED == fe_cases.STAGING[-1][0] + 1 and "ring_%d" % fe_cases.RING_REFUSED in fe_cases.CASES
    assert all(s[0].split("@")[0] in fe_cases.CASES for s in fe_cases.SPEC_SEQUENCE)
    # every sweep keeps clear of the azimuth wrap thresholds (:189-203): nothing before -2.8 or behind 2.8 rad
    for name in fe_cases.CASES:
        raw = fe_cases.get(name)[0]
        keep = fe_reference.a1_filter(raw)
        if keep.any():
            ori = -np.arctan2(raw[keep, 1].astype(np.float64), raw[keep, 0].astype(np.float64))
            assert ori.min() >= -2.8001 and ori.max() <= 2.8001 and np.all(np.diff(ori) >= -1e-6), name


def _ring_counts(name):
    raw, prm, _ = fe_cases.get(name)
    c, r = fe_reference.census(name)
    return prm["n_scans"], ([] if r is None else [int(v) for v in r["rb"]["ring_count"]]), len(raw)


def test_speculative_sequence_routes():
    """the route of every sweep of SPEC_SEQUENCE -- speculative, fallen back, synchronous, refused -- and its sectors per staging window,
    from the restatement's ring counts through fe_cases.spec_route (the launcher's decision restated): the GPU test cannot see the route,
    this is its proof.  The window edge: guess + 12 stays speculative, guess + 13 falls back."""
    state = fe_cases.spec_route(None, *_ring_counts("spec_1000"))[2]
    assert state == (16, 1000)
    routes = set()
    for step, route, group in fe_cases.SPEC_SEQUENCE:
        got, g, state = fe_cases.spec_route(state, *_ring_counts(step.split("@")[0]))
        assert (got, g) == (route, group), (step, got, g)
        routes.add((got, g))
    assert {("spec", 6), ("spec", 3), ("fallback", 6), ("sync", 6), ("refused", 0), ("empty", 0)} <= routes
    # every case after itself (test_speculative_after_itself): speculative, and for a largest ring of 2555 .. 3256, 5159 .. 6512, 7764 .. 9768 with
    # fewer sectors per window than the synchronous launch
    fewer = []
    for name, case in fe_cases.CASES.items():
        ns, rc, n_raw = _ring_counts(name)
        if case.refused or not rc:
            continue
        first = fe_cases.spec_route(None, ns, rc, n_raw)
        second = fe_cases.spec_route(first[2], ns, rc, n_raw)
        assert first[0] == "sync" and second[0] == "spec", name
        if second[1] != first[1]:
            fewer.append((name, first[1], second[1]))
    assert ("ring_3256", 6, 3) in fewer and ("ring_6512", 3, 2) in fewer and ("ring_9768", 2, 1) in fewer and ("spec_3000", 6, 3) in fewer
