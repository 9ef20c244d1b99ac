"""The LM solve as ONE resident launch (k_lm_solve, the default) against the chain of step launches (RGC_LM_IMPL=chained): the same state
machine, the same rows, the same fixed-order fold -- so every comparison here is bit for bit, no tolerance anywhere.  Needs an MI355X: -m gpu.

A workgroup of the resident solve holds V = 1 virtual block of 256 points, so the scan sizes 256 V - 1, 256 V, 256 V + 1 of the row and
workgroup edges are 255, 256, 257."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V = 1
EDGE_SIZES = sorted({64, 255, 256, 257, 256 * V - 1, 256 * V, 256 * V + 1, 2000})


@pytest.fixture(scope="module")
def reg_mod():
    from rgc_slam_amd import registration
    return registration


def _ctx(reg_mod, monkeypatch, impl, give_up_at=None):
    """a context of the given route (the environment is read when the context is created)"""
    if impl is None:
        monkeypatch.delenv("RGC_LM_IMPL", raising=False)
    else:
        monkeypatch.setenv("RGC_LM_IMPL", impl)
    if give_up_at is None:
        monkeypatch.delenv("RGC_LM_GIVE_UP_AT", raising=False)
    else:
        monkeypatch.setenv("RGC_LM_GIVE_UP_AT", str(give_up_at))
    v = reg_mod.odometer_vgicp(0)
    monkeypatch.delenv("RGC_LM_IMPL", raising=False)
    monkeypatch.delenv("RGC_LM_GIVE_UP_AT", raising=False)
    return v


def _result(v):
    st = v.stats()
    return dict(T=v.getFinalTransformation().tobytes(), H=v.getFinalHessian().tobytes(), iters=v.nr_iterations, conv=v.hasConverged(),
                failed=v.lm_failed, fit=np.float64(v.getFitnessScore()).tobytes(), n_lin=st["n_linearize"], n_err=st["n_error"], n_corr=st["n_corr"])


def _solve(v, fx, n, guess):
    v.setInputSource(fx["src"][:n])
    v.align(guess, want_output=False)
    return _result(v)


def _far(fx):
    import rgc_slam_amd.synth as synth
    return (synth.se3(synth.rot_zyx(0.06, 0.0, 0.0), [0.9, -0.5, 0.05]) @ fx["guess"].astype(np.float64)).astype(np.float32)


_REF = {}


def _run(reg_mod, fx, monkeypatch, impl, sizes, give_up_at=None):
    """a fresh context of the given route, the fixture's map, then one solve per entry of `sizes` (the first n points of the fixture's scan)
    -> the results and the context's lm_fallbacks after each solve.  A context steers its next scan's grid by the last one's crowding, so
    two routes are compared over the SAME sequence of scans on a fresh context each."""
    v = _ctx(reg_mod, monkeypatch, impl, give_up_at)
    v.setInputTarget(fx["tgt"])
    res, fb = [], []
    for n in sizes:
        res.append(_solve(v, fx, n, fx["guess"]))
        fb.append(v.stats()["lm_fallbacks"])
    v.close()
    return res, fb


def _chained(reg_mod, fx, monkeypatch, sizes):
    """the chained route's results for that sequence (computed once per sequence; the tests only read them)"""
    key = tuple(sizes)
    if key not in _REF:
        _REF[key], fb = _run(reg_mod, fx, monkeypatch, "chained", sizes)
        assert fb == [0] * len(sizes)
    return _REF[key]


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_row_and_workgroup_edges(reg_mod, fx_reg, monkeypatch, n):
    """one virtual block, one workgroup alone (nobody to wait for), a last workgroup with a single point, several workgroups"""
    got, fb = _run(reg_mod, fx_reg, monkeypatch, None, [n])
    print(n, {k: got[0][k] for k in ("iters", "conv", "failed", "n_lin", "n_err", "n_corr")})
    assert got == _chained(reg_mod, fx_reg, monkeypatch, [n])
    assert fb == [0]


def test_as_many_workgroups_as_compute_units(reg_mod, monkeypatch):
    """the edge of the rule that picks the route, linearize_blocks(n) == the device's CU count: scans of 256 (cu - 1) + 1 and 256 cu points fill every
    CU with one workgroup of the resident launch (the second to its last lane), 256 cu + 1 points need one workgroup more and go through the chained
    launches by rule.  Each against RGC_LM_IMPL=chained bit for bit on a 100 k-point map; which route ran is read with the hook: a context made with
    RGC_LM_GIVE_UP_AT=0 counts one fallback per resident solve and none for a solve that was chained anyway -- and the same bits either way"""
    import subprocess
    import sys
    import rgc_slam_amd.synth as synth
    # the CU count as torch reports it, not as the library read it; asked in a child process: this one's HIP runtime is the one the library bound to
    # when it was loaded, and torch's own cannot start beside it (bench.py imports torch first for the same reason)
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    cu = int(r.stdout.split()[-1])
    sizes = [256 * (cu - 1) + 1, 256 * cu, 256 * cu + 1]
    world, tgt = synth.make_world_and_map(100000, seed=synth.SEED + 7)
    T_true = synth.se3(synth.rot_zyx(0.01, 0.002, -0.001), [0.08, 0.03, 0.002])
    src = synth.make_scan_n(world, T_true, sizes[-1], seed=synth.SEED + 7)["xyz"]
    assert len(src) == sizes[-1]
    fx = dict(tgt=tgt, src=src, guess=np.eye(4, dtype=np.float32))
    ref = _chained(reg_mod, fx, monkeypatch, sizes)
    got, fb = _run(reg_mod, fx, monkeypatch, None, sizes)
    print(cu, sizes, [{k: g[k] for k in ("iters", "conv", "failed", "n_lin", "n_err", "n_corr")} for g in got])
    assert got == ref
    assert fb == [0, 0, 0]                      # alone, no solve of the default route gives up
    hooked, fb = _run(reg_mod, fx, monkeypatch, None, sizes, give_up_at=0)
    assert hooked == ref
    assert np.diff([0] + fb).tolist() == [1, 1, 0]


@pytest.mark.parametrize("max_it,lm_it,far", [(0, 10, False), (1, 10, False), (2, 10, False), (3, 10, False), (25, 1, True), (25, 2, True),
                                              (40, 10, True)])
def test_the_solves_ends(reg_mod, fx_reg, monkeypatch, max_it, lm_it, far):
    """test_lm_edge_settings' parameters: the iteration cap, rejected tries, LM_MODE_B and "lm not converged" from the far guess.  Each
    setting twice in a row on one context: the second solve meets the first one's flags and rows."""
    guess = _far(fx_reg) if far else fx_reg["guess"]
    res = {}
    for impl in ("chained", None):
        v = _ctx(reg_mod, monkeypatch, impl)
        v.setMaximumIterations(max_it)
        v._p.lm_max_iterations = lm_it
        v._push()
        v.setInputTarget(fx_reg["tgt"])
        res[impl] = [_solve(v, fx_reg, 2000, guess) for rep in range(2)]
        assert v.stats()["lm_fallbacks"] == 0
        v.close()
    print(max_it, lm_it, far, {k: res[None][0][k] for k in ("iters", "conv", "failed", "n_lin", "n_err", "n_corr")})
    assert res[None] == res["chained"]


@pytest.mark.parametrize("method", ["DIRECT7", "DIRECT27"])
def test_correspondence_modes(reg_mod, fx_reg, monkeypatch, method):
    res = {}
    for impl in ("chained", None):
        v = _ctx(reg_mod, monkeypatch, impl)
        v.setNeighborSearchMethod(getattr(reg_mod.NeighborSearchMethod, method))
        v.setInputTarget(fx_reg["tgt"])
        res[impl] = _solve(v, fx_reg, 2000, fx_reg["guess"])
        assert v.stats()["lm_fallbacks"] == 0
        v.close()
    assert res[None] == res["chained"]


def test_many_solves_on_one_context(reg_mod, fx_reg, monkeypatch):
    """sixty solves with alternating scan sizes: no flag or row of an earlier solve is taken for this one's"""
    sizes = [(257, 2000)[k & 1] for k in range(60)]
    got, fb = _run(reg_mod, fx_reg, monkeypatch, None, sizes)
    ref = _chained(reg_mod, fx_reg, monkeypatch, sizes)
    assert [k for k in range(60) if got[k] != ref[k]] == []
    assert fb == [0] * 60


def test_dependent_sequence_on_two_contexts(reg_mod, fx_reg, monkeypatch):
    """the path the headline runs: align_begin / align_end_reframe on two contexts taking turns, the early pose, the chained score.  The
    fixture's map is the world map, the scans are the fixture's scan moved by small known poses."""
    import bench
    import rgc_slam_amd.synth as synth
    tgt, src = fx_reg["tgt"], fx_reg["src"]
    scans = []
    for i in range(6):
        M = synth.se3(synth.rot_zyx(0.004 * i, -0.001 * i, 0.0005 * i), [0.03 * i, -0.01 * i, 0.002 * i])
        scans.append((src.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32))
    out = {}
    for impl in ("chained", None):
        pv = reg_mod.PipelinedVGICP(0, depth=2, contexts=[_ctx(reg_mod, monkeypatch, impl), _ctx(reg_mod, monkeypatch, impl)])
        v = pv.v[0]
        def to_dev(xyz):
            a = np.zeros((xyz.shape[0], 4), np.float32); a[:, :3] = xyz
            p = v.device_alloc(a.nbytes); v.upload(p, a); return p
        d_map, d_scans = to_dev(tgt), [to_dev(s) for s in scans]
        seq = bench.DependentSequence(pv.v, d_map, len(tgt), d_scans, [len(s) for s in scans])
        motions, worlds, _ = seq.run(0, 6, np.eye(4), fx_reg["guess"], True)
        out[impl] = (motions, worlds, [w.stats()["lm_fallbacks"] for w in pv.v])
        seq.close()
        for p in [d_map] + d_scans:
            v.device_free(p)
        for w in pv.v:
            w.close()
    for a, b in zip(out[None][0], out["chained"][0]):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(out[None][1], out["chained"][1]):
        assert a.tobytes() == b.tobytes()
    assert out[None][2] == [0, 0]


@pytest.mark.parametrize("at", [0, 1, 3])
def test_the_way_out(reg_mod, fx_reg, monkeypatch, at):
    """RGC_LM_GIVE_UP_AT: workgroup 0 gives up at that try without waiting, the others leave when they see its word; the host finds no
    result and solves again through the chained launches -- the same bits, one fallback per solve"""
    sizes = [2000, 257, 2000]
    got, fb = _run(reg_mod, fx_reg, monkeypatch, None, sizes, give_up_at=at)
    assert got == _chained(reg_mod, fx_reg, monkeypatch, sizes)
    assert fb == [1, 2, 3]


def test_a_context_that_gives_up_beside_one_that_does_not(reg_mod, fx_reg, monkeypatch):
    ref = _chained(reg_mod, fx_reg, monkeypatch, [2000, 2000, 2000])
    a = _ctx(reg_mod, monkeypatch, None, give_up_at=1)
    b = _ctx(reg_mod, monkeypatch, None)
    for v in (a, b):
        v.setInputTarget(fx_reg["tgt"])
    for k in range(3):
        for v in (a, b):
            assert _solve(v, fx_reg, 2000, fx_reg["guess"]) == ref[k], k
    assert a.stats()["lm_fallbacks"] == 3 and b.stats()["lm_fallbacks"] == 0
    a.close(); b.close()


def test_lazy_target_whose_miss_flag_trips(reg_mod, fx_reg, monkeypatch):
    """the lazy target's miss flag rides home with the resident solve's state as it does with the chained one's: guesses turned and moved so
    far from the answer that the solve carries the scan's far points more than the two voxels of margin away from where they fell at the guess
    -- look-ups land on occupied voxels outside the part that was built and the solve is repeated on the completed map"""
    import rgc_slam_amd.synth as synth
    g0 = fx_reg["guess"].astype(np.float64)
    guesses = [_far(fx_reg)] + [(synth.se3(synth.rot_zyx(yaw, 0.0, 0.0), t) @ g0).astype(np.float32)
                                for yaw, t in ((0.1, [0.5, 0.0, 0.0]), (-0.1, [0.0, 0.8, 0.0]), (0.15, [1.5, -1.0, 0.0]), (0.0, [2.8, 0.0, 0.0]), (0.0, [0.0, -3.2, 0.0]))]
    res = {}
    for impl in ("chained", None):
        v = _ctx(reg_mod, monkeypatch, impl)
        v.setLazyTarget(2)
        got, misses = [], []
        for g in guesses:
            v.setInputTarget(fx_reg["tgt"])
            got.append(_solve(v, fx_reg, 2000, g))
            misses.append(v.stats()["lazy_misses"])
        res[impl] = (got, misses, v.stats()["lm_fallbacks"])
        v.close()
    print("lazy misses after each solve", res["chained"][1], res[None][1])
    assert res["chained"][1][-1] >= 1
    assert res[None] == res["chained"]
