"""VGICP under NeighborSearchMethod::DIRECT_RADIUS (rgc_set_neighbor_search) on every route it can take, against tests/vgicp_reference.py run over
the numpy offset table of tests/vgicp_radius_reference.py.  As in tests/test_gpu_voxel_lookup.py the reference takes the covariances the GPU itself
reports, and that file's bars hold: correspondence counts exact, cost / H / b / compute_error 1e-9 (vr.rel); whole solves by
_against_oracle_solve's bars (iterations and converged equal, 1e-4 m / 1e-4 rad, the final H 1e-6).

  * every shell of the table (radii 0.999, 1.4133, 1.7311, 2.0, 3.0: 7, 19, 27, 33, 123 offsets) at resolutions 0.3 / 1.0 / 1.7 on the tuned route
    and on the general route (RGC_FORCE_GENERAL=1 with MIN_EIG + MULTIPLICATIVE; RBF covariances once);
  * source sizes 20 / 255 / 256 / 257 / 1500 at 33 offsets (no multiple of a lane group; one workgroup more or less) and 485 offsets on 64 points;
  * the grid's edges: one occupied voxel under a cube of sources (the count IS the table's size, every other look-up leaves the grid), a 3-D
    checkerboard, a map 1e4 m from the origin;
  * r = 0 / 1.0 / 1.7311 against DIRECT1 / DIRECT7 / DIRECT27 on the same context; the frozen list under a switched method; the setters' refusals,
    the refusal with a solve in flight, get / modify / set of rgc_params;
  * whole solves: r = 1.7311 against the oracle's DIRECT27 solve (align, align_begin / align_end), r = 2.0 against a closed loop of
    tests/lm_reference.py over the numpy linearisation, whose own decisions keep a margin from their thresholds (asserted from the reference alone);
  * lazy, re-framed, shared and map-bound targets bit for bit against a plain one; two runs and host against device inputs bit for bit; the C++
    adaptor.

Clouds: 6 000 target and 1 500 source points.  Cost on one MI355X: about 7 s, most of it the references on the CPU.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import lm_reference as lm
import vgicp_radius_reference as vrr
import vgicp_reference as vr
from test_gpu_voxel_lookup import _against_oracle_solve, _check_linearize, _checkerboard, _oracle_solve

pytestmark = pytest.mark.gpu

RADIUS = 3                                           # RGC_DIRECT_RADIUS
SHELLS = [0.999, 1.4133, 1.7311, 2.0, 3.0]
CL = {}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reg_mod():
    from rgc_slam_amd import registration
    return registration


@pytest.fixture(scope="module", autouse=True)
def clouds():
    import rgc_slam_amd.synth as synth
    world, tgt = synth.make_world_and_map(6000, seed=synth.SEED + 71)
    T_true = synth.se3(synth.rot_zyx(0.012, 0.002, -0.001), [0.11, 0.03, 0.002])
    CL.update(tgt=tgt, src=synth.make_scan_n(world, T_true, 1500, seed=synth.SEED + 71)["xyz"])
    CL["T_lin"] = synth.se3(synth.rot_zyx(0.015, -0.004, 0.003), [0.09, 0.05, -0.01])
    CL["T_err"] = synth.se3(synth.rot_zyx(0.0155, -0.0041, 0.0028), [0.094, 0.046, -0.012])
    yield
    CL.clear()


def _odo(reg_mod, res, radius=None, mode=None, reg=None):
    v = reg_mod.odometer_vgicp(0)
    v.setResolution(res)
    if radius is not None:
        v.setNeighborSearchMethod(RADIUS, radius)
    if reg is not None:
        v.setRegularizationMethod(reg)
    if mode is not None:
        v.setVoxelAccumulationMode(mode)
    return v


def _shells(v, tgt, src, res, mode, what):
    """every shell on one context, against the reference; the counts must grow with the table (asserted from the reference's own counts)"""
    table, counts = None, []
    for r in SHELLS:
        v.setNeighborSearchMethod(RADIUS, r)
        assert v.getNeighborSearchMethod() == (RADIUS, r)
        table, corr = _check_linearize(v, tgt, src, res, vrr.method(r), mode, CL["T_lin"], CL["T_err"], f"{what} r={r}", table)
        counts.append(len(corr["src"]))
    assert all(a < b for a, b in zip(counts, counts[1:])), (what, counts)
    print(f"{what}: correspondences {counts}")


@pytest.mark.parametrize("res", [0.3, 1.0, 1.7])
def test_every_shell_tuned_route(reg_mod, res):
    v = _odo(reg_mod, res)
    v.setInputTarget(CL["tgt"]); v.setInputSource(CL["src"])
    _shells(v, CL["tgt"], CL["src"], res, "ADDITIVE", f"tuned res={res}")
    v.close()


@pytest.mark.parametrize("res", [0.3, 1.0, 1.7])
def test_every_shell_general_route(reg_mod, monkeypatch, res):
    monkeypatch.setenv("RGC_FORCE_GENERAL", "1")
    v = _odo(reg_mod, res, mode=reg_mod.FastVGICP.VOXEL_MULTIPLICATIVE, reg=reg_mod.FastVGICP.REG_MIN_EIG)
    monkeypatch.delenv("RGC_FORCE_GENERAL")
    v.setInputTarget(CL["tgt"]); v.setInputSource(CL["src"])
    _shells(v, CL["tgt"], CL["src"], res, "MULTIPLICATIVE", f"general res={res}")
    v.close()


def test_every_shell_rbf_covariances(reg_mod):
    v = _odo(reg_mod, 1.0)
    v.setNearestNeighborSearchMethod(reg_mod.FastVGICP.NearestNeighborMethod.GPU_RBF_KERNEL)
    v.setInputTarget(CL["tgt"]); v.setInputSource(CL["src"])
    _shells(v, CL["tgt"], CL["src"], 1.0, "ADDITIVE", "RBF res=1.0")
    v.close()


@pytest.mark.parametrize("n_src,radius", [(20, 2.0), (255, 2.0), (256, 2.0), (257, 2.0), (1500, 2.0), (64, 4.9)])
def test_group_and_block_boundaries(reg_mod, n_src, radius):
    """33 offsets are no multiple of any lane-group size; 255 / 256 / 257 points end a workgroup of every group size one point short, full and one
    over; 485 offsets: the largest table"""
    src = CL["src"][:n_src]
    assert len(vrr.offsets(radius)) == vrr.COUNTS[radius]
    for general in (False, True):
        v = _odo(reg_mod, 1.0, radius, reg=reg_mod.FastVGICP.REG_FROBENIUS if general else None)
        v.setInputTarget(CL["tgt"]); v.setInputSource(src)
        _, corr = _check_linearize(v, CL["tgt"], src, 1.0, vrr.method(radius), "ADDITIVE", CL["T_lin"], CL["T_err"],
                                   f"{'general' if general else 'tuned'} n={n_src} r={radius}")
        assert len(corr["src"]) > n_src
        v.close()


def _cube_sources(radius, res):
    """one point at the centre of every cell of the (2 ceil(r) + 3)^3 cube around cell (0, 0, 0)"""
    h = int(math.ceil(radius)) + 1
    g = np.stack(np.meshgrid(*[np.arange(-h, h + 1)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return ((g + 1.0) * res).astype(np.float32)      # cell c covers [(c + 0.5) res, (c + 1.5) res)


@pytest.mark.parametrize("radius", [1.0, 1.5, 2.0, 3.0])
def test_grid_edges_one_voxel_and_a_checkerboard(reg_mod, radius):
    res = 1.0
    rng = np.random.default_rng(int(radius * 10))
    src = _cube_sources(radius, res)
    assert len(src) == (2 * int(math.ceil(radius)) + 3) ** 3
    one = ((0.5 + rng.uniform(0.1, 0.9, (40, 3))) * res).astype(np.float32)          # 40 points in cell (0, 0, 0): a 1 x 1 x 1 grid
    v = _odo(reg_mod, res, radius)
    v.setInputTarget(one); v.setInputSource(src)
    _, corr = _check_linearize(v, one, src, res, vrr.method(radius), "ADDITIVE", np.eye(4), np.eye(4), f"one voxel r={radius}")
    assert v.num_correspondences == len(vrr.offsets(radius)) == len(corr["src"])     # a source in cell c reaches the voxel iff -c is in the table
    board = _checkerboard(res, rng, lo=-3, hi=3)
    v.setInputTarget(board)
    _check_linearize(v, board, src, res, vrr.method(radius), "ADDITIVE", np.eye(4), CL["T_err"], f"checkerboard r={radius}")
    v.close()


def test_far_offset_map(reg_mod):
    off = np.float32([1.0e4, -1.0e4, 3.0e3])
    tgt, src = CL["tgt"] + off, CL["src"] + off
    S = off.astype(np.float64)
    Tl, Te = CL["T_lin"].copy(), CL["T_err"].copy()
    Tl[:3, 3] += S - Tl[:3, :3] @ S
    Te[:3, 3] += S - Te[:3, :3] @ S
    v = _odo(reg_mod, 0.75, 2.0)
    v.setInputTarget(tgt); v.setInputSource(src)
    _check_linearize(v, tgt, src, 0.75, vrr.method(2.0), "ADDITIVE", Tl, Te, "far r=2.0")
    v.close()


def test_equivalences_with_the_fixed_methods(reg_mod):
    tgt, src, res = CL["tgt"], CL["src"], 0.75
    v = _odo(reg_mod, res)
    v.setInputTarget(tgt); v.setInputSource(src)
    table = None
    for radius, name, code in ((0.0, "DIRECT1", 2), (1.0, "DIRECT7", 1), (1.7311, "DIRECT27", 0)):
        v.setNeighborSearchMethod(RADIUS, radius)
        table, ca = _check_linearize(v, tgt, src, res, vrr.method(radius), "ADDITIVE", CL["T_lin"], CL["T_err"], f"r={radius}", table)
        n_radius = v.num_correspondences
        v.setNeighborSearchMethod(code)
        _, cb = _check_linearize(v, tgt, src, res, name, "ADDITIVE", CL["T_lin"], CL["T_err"], name, table)
        assert n_radius == v.num_correspondences == len(ca["src"]) == len(cb["src"]), (radius, name)
    v.close()


def test_frozen_list(reg_mod):
    tgt, src, res = CL["tgt"], CL["src"], 1.0
    v = _odo(reg_mod, res, 2.0)
    v.setInputTarget(tgt); v.setInputSource(src)
    table = vr.voxel_table(tgt, v.getTargetCovariances(), res, "ADDITIVE")
    sc = v.getSourceCovariances()
    v.linearize(CL["T_lin"])
    _, _, _, corr = vr.linearize(src, sc, table, CL["T_lin"], res, vrr.method(2.0))
    want = vr.compute_error(src, table, corr, CL["T_err"])
    n = v.num_correspondences
    for switch in ((2, -1.0), (RADIUS, 1.0), (0, 7.0), (RADIUS, 3.0)):                # DIRECT1, radius 1.0, DIRECT27, radius 3.0: still the 2.0 list
        v.setNeighborSearchMethod(*switch)
        assert vr.rel(v.compute_error(CL["T_err"]), want) <= 1e-9 and v.num_correspondences == n == len(corr["src"]), switch
    v.setInputSource(src)                                                             # a new source drops the list
    with pytest.raises(reg_mod.RgcError):
        v.compute_error(CL["T_err"])
    v.setNeighborSearchMethod(RADIUS, 2.0)
    v.linearize(CL["T_lin"])
    assert vr.rel(v.compute_error(CL["T_err"]), want) <= 1e-9
    v.close()


def test_setters(reg_mod, monkeypatch):
    from rgc_slam_amd import _lib
    monkeypatch.delenv("RGC_LM_IMPL", raising=False)
    tgt, src = CL["tgt"], CL["src"]
    v = _odo(reg_mod, 1.0)
    L, h = v._L, v._h
    assert v.getNeighborSearchMethod() == (2, 0.0)                                    # a new context: DIRECT1, radius 0.0
    v.setNeighborSearchMethod(RADIUS, 1.5)
    for bad in (5.0, math.nan, math.inf, -0.5):
        with pytest.raises(reg_mod.RgcError) as e:
            v.setNeighborSearchMethod(RADIUS, bad)
        assert e.value.status == -1 and v.getNeighborSearchMethod() == (RADIUS, 1.5), bad
    for bad_method in (-1, 4):
        assert L.rgc_set_neighbor_search(h, bad_method, 1.0) == -1 and v.getNeighborSearchMethod() == (RADIUS, 1.5)
    assert L.rgc_set_neighbor_search(None, 3, 1.0) == -1
    m, r = C.c_int(0), C.c_double(0)
    assert L.rgc_get_neighbor_search(h, None, C.byref(r)) == -1 and L.rgc_get_neighbor_search(h, C.byref(m), None) == -1
    assert L.rgc_get_neighbor_search(None, C.byref(m), C.byref(r)) == -1
    for code in (0, 1, 2):                                                            # any radius, ignored; the stored one stays
        for any_radius in (-1.0, math.nan, 99.0):
            v.setNeighborSearchMethod(code, any_radius)
            assert v.getNeighborSearchMethod() == (code, 1.5)
    # get, modify, set of the parameter block keeps method 3 and the radius
    v.setNeighborSearchMethod(RADIUS, 2.0)
    p = _lib.Params()
    assert L.rgc_get_params(h, C.byref(p)) == 0 and p.neighbor_method == RADIUS
    p.max_iterations = 30
    assert L.rgc_set_params(h, C.byref(p)) == 0 and v.getNeighborSearchMethod() == (RADIUS, 2.0)
    v.setMaximumIterations(25)                                                        # the adaptor pushes its own block: the method stays
    assert v.getNeighborSearchMethod() == (RADIUS, 2.0)
    p.neighbor_method = 4
    assert L.rgc_set_params(h, C.byref(p)) == -1 and v.getNeighborSearchMethod() == (RADIUS, 2.0)
    # the block carries no radius: it keeps the radius method while that is selected, it cannot select it
    p.neighbor_method, p.max_iterations = 1, 25
    assert L.rgc_set_params(h, C.byref(p)) == 0 and v.getNeighborSearchMethod() == (1, 2.0)
    p.neighbor_method = RADIUS
    assert L.rgc_set_params(h, C.byref(p)) == -1 and v.getNeighborSearchMethod() == (1, 2.0)
    # refused between align_begin and align_end on the device LM route, and the pending solve unharmed
    v.setNeighborSearchMethod(1)
    v.setInputTarget(tgt); v.setInputSource(src)
    I4 = np.eye(4, dtype=np.float32)
    v.align(I4, want_output=False)
    want = (v.getFinalTransformation().copy(), v.nr_iterations)
    v.align_begin(I4)
    with pytest.raises(reg_mod.RgcError):
        v.setNeighborSearchMethod(RADIUS, 2.0)
    with pytest.raises(reg_mod.RgcError):
        v.setNeighborSearchMethod(0)
    assert v.getNeighborSearchMethod() == (1, 2.0)
    v.align_end()
    assert np.array_equal(v.getFinalTransformation(), want[0]) and v.nr_iterations == want[1]
    # ... and under the radius method itself, where align_begin has solved at once
    v.setNeighborSearchMethod(RADIUS, 2.0)
    v.align_begin(I4)
    with pytest.raises(reg_mod.RgcError):
        v.setNeighborSearchMethod(RADIUS, 1.0)
    v.align_end()
    assert v.getNeighborSearchMethod() == (RADIUS, 2.0) and v.hasConverged()
    v.close()


@pytest.mark.parametrize("impl", ["device", "host"])
def test_solve_r17311_against_the_oracles_direct27(reg_mod, orc, monkeypatch, impl):
    """the table at 1.7311 is DIRECT27's: the oracle's DIRECT27 solve is the reference; whatever RGC_LM_IMPL says the host loop drives it"""
    if impl == "host":
        monkeypatch.setenv("RGC_LM_IMPL", "host")
    else:
        monkeypatch.delenv("RGC_LM_IMPL", raising=False)
    o = _oracle_solve(orc, CL["tgt"], CL["src"], "DIRECT27")
    v = _odo(reg_mod, 1.0, 1.7311)
    v.setInputTarget(CL["tgt"]); v.setInputSource(CL["src"])
    I4 = np.eye(4, dtype=np.float32)
    v.align(I4, want_output=False)
    _against_oracle_solve(v, o, f"align r=1.7311 {impl}")
    one = (v.getFinalTransformation().copy(), v.getFinalHessian().copy(), v.nr_iterations)
    if impl == "device":
        v.align_begin(I4)
        v.align_end()
        _against_oracle_solve(v, o, "align_begin / align_end r=1.7311")
        assert np.array_equal(v.getFinalTransformation(), one[0]) and np.array_equal(v.getFinalHessian(), one[1]) and v.nr_iterations == one[2]
    v.close()


def _reference_solve(src, sc, table, res, key, guess, prm):
    """LsqRegistration::computeTransformation (lsq_registration_impl.hpp:53-79) over step_lm (:125-172), the scalar step from lm_reference, the
    linearisation from vgicp_reference.  -> x0, final H, iterations, converged, margins: per decision how far its quantity was from its threshold"""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    x0 = lm.ld(np.asarray(guess, np.float32).astype(np.float64).reshape(4, 4))
    lam, Hfin, conv, iters, margins = lm.LD(-1), np.eye(6), False, 0, []
    for it in range(prm.max_iterations):
        if conv:
            break
        iters = it + 1
        y0, H, b, corr = vr.linearize(src, sc, table, f64(x0), res, key)
        if lam < 0:
            lam = lm.LD(prm.lm_init_lambda_factor) * lm.LD(np.abs(np.diag(H)).max())
        nu, ok, delta = 2, False, None
        for k in range(prm.lm_max_iterations):
            d, delta, xi = lm.lm_try(H, b, lam, x0)
            yi = vr.compute_error(src, table, corr, f64(xi))
            rho = float((lm.LD(y0) - lm.LD(yi)) / (d @ (lam * d - lm.ld(b))))
            margins.append(("rho", abs(rho)))
            # the cost's decrease in units of what two fp64 sums of len(corr) terms can be off by in the worst case (n 2^-53 of the cost each)
            margins.append(("decrease", abs(float(y0) - float(yi)) / (len(corr["src"]) * 2.0 ** -52 * abs(float(y0)))))
            verdict, x0, lam, nu, Hw = lm.step_lm_try(x0, lam, nu, k, H, b, y0, d, delta, xi, yi, prm.rotation_eps, prm.translation_eps,
                                                      prm.lm_max_iterations)
            if Hw is not None:
                Hfin = f64(Hw).reshape(6, 6)
            if verdict in (lm.ACCEPT, lm.END_OUTER):
                ok = True
                break
            if verdict == lm.NOT_CONVERGED:
                break
        if not ok:
            return f64(x0), Hfin, iters, False, margins, True
        D = f64(delta)
        m = max(float((np.abs(D[:3, :3] - np.eye(3)) / prm.rotation_eps).max()), float((np.abs(D[:3, 3]) / prm.translation_eps).max()))
        margins.append(("converged", abs(m - 1.0)))
        conv = lm.is_converged(delta, prm.rotation_eps, prm.translation_eps)
    return f64(x0), Hfin, iters, conv, margins, False


def test_solve_r2_against_a_closed_reference_loop(reg_mod):
    from rgc_slam_amd import _lib
    from test_gpu_voxel_lookup import _rot_angle
    tgt, src, res = CL["tgt"], CL["src"], 1.0
    v = _odo(reg_mod, res, 2.0)
    v.setTransformationEpsilon(1e-4)      # (the last accepted step of a solve down to 1e-6 m lowers the cost by less than its sums' rounding: no margin)
    v.setInputTarget(tgt); v.setInputSource(src)
    prm = _lib.Params()
    assert v._L.rgc_get_params(v._h, C.byref(prm)) == 0
    table = vr.voxel_table(tgt, v.getTargetCovariances(), res, "ADDITIVE")
    guess = np.eye(4, dtype=np.float32)
    x0, Hfin, iters, conv, margins, failed = _reference_solve(src, v.getSourceCovariances(), table, res, vrr.method(2.0), guess, prm)
    print(f"reference: {iters} iterations, converged {conv}, margins {[(n, float('%.3g' % m)) for n, m in margins]}")
    # The margins, from the reference alone.  A try is accepted on the SIGN of rho = (y0 - yi) / (model decrease): both sides sum the same terms in
    # fp64, in another order, so y0 - yi can differ by the sums' rounding at most -- the decrease must be a hundred times the worst case of that,
    # and rho itself away from 0.  An outer iteration ends on max(|delta - I| / eps) < 1: the step solves a system whose entries agree to 1e-9
    # (the bars above), far inside 5 % of the threshold.  Every decision of the loop is then the GPU's decision too.
    assert not failed and conv and 2 <= iters < prm.max_iterations
    assert all(m > 1e-3 for n, m in margins if n == "rho"), margins
    assert all(m > 100.0 for n, m in margins if n == "decrease"), margins
    assert all(m > 0.05 for n, m in margins if n == "converged"), margins
    for how in ("align", "begin_end"):
        if how == "align":
            v.align(guess, want_output=False)
        else:
            v.align_begin(guess)
            v.align_end()
        T = v.getFinalTransformation()
        dt, dth = float(np.abs(T[:3, 3] - x0[:3, 3]).max()), _rot_angle(T[:3, :3], x0[:3, :3])
        print(f"{how}: iterations {v.nr_iterations} / {iters}, dt {dt:.1e} m, dtheta {dth:.1e} rad, H {vr.rel(v.getFinalHessian(), Hfin):.1e}")
        assert v.nr_iterations == iters and v.hasConverged() == conv and not v.lm_failed, how
        assert dt <= 1e-4 and dth <= 1e-4, how
        assert vr.rel(v.getFinalHessian(), Hfin) <= 1e-6, how
    v.close()


def test_lazy_reframed_shared_and_map_bound_targets(reg_mod):
    import bench
    import rgc_slam_amd.synth as synth
    from rgc_slam_amd import local_map
    tgt, src = CL["tgt"], CL["src"]
    I4 = np.eye(4, dtype=np.float32)
    far = I4.copy(); far[:3, 3] = [0.9, -0.7, 0.2]

    def solve(v, guess):
        v.align(guess, want_output=False)
        return v.getFinalTransformation(), v.nr_iterations, v.getFinalHessian()

    def same(a, b):
        return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])

    want = {}
    for g, G in (("near", I4), ("far", far)):
        plain = _odo(reg_mod, 1.0, 2.0)
        plain.setInputTarget(tgt); plain.setInputSource(src)
        want[g] = solve(plain, G)
        if g == "near":                                              # shared: a second context on the plain one's target
            sh = _odo(reg_mod, 1.0, 2.0)
            sh.shareTargetFrom(plain)
            sh.setInputSource(src)
            assert same(solve(sh, I4), want["near"]), "shared"
            sh.close()
        plain.close()
    for margin in (1, 2):                                            # lazy: completed before the solve, the full build's results
        for g, G in (("near", I4), ("far", far)):
            lz = _odo(reg_mod, 1.0, 2.0)
            lz.setLazyTarget(margin)
            lz.setInputTarget(tgt); lz.setInputSource(src)
            assert same(solve(lz, G), want[g]), ("lazy", margin, g)
            lz.close()
    n = len(tgt)                                                     # re-framed
    a = np.zeros((n, 4), np.float32); a[:, :3] = tgt
    q, t = bench.world_to_body(synth.se3(synth.rot_zyx(0.3, 0.01, -0.02), [1.5, -1.0, 0.1]))
    v = _odo(reg_mod, 1.0, 2.0)
    d_map, d_body = v.device_alloc(a.nbytes), v.device_alloc(a.nbytes)
    v.upload(d_map, a)
    v.setInputTargetReframed(d_map, n, 16, q, t, d_body)
    v.setInputSource(src)
    body = v.download(d_body, (n, 4))[:, :3].copy()
    p2 = _odo(reg_mod, 1.0, 2.0)
    p2.setInputTarget(body); p2.setInputSource(src)
    assert same(solve(v, I4), solve(p2, I4)), "re-framed"
    p2.close()
    v.device_free(d_map); v.device_free(d_body)
    v.close()
    m_ctx = _odo(reg_mod, 1.0, 2.0)                                  # map-bound
    m = local_map.RollingLocalMap(m_ctx)
    m.reset(np.zeros(3))
    m.insert(np.c_[tgt, np.zeros(n, np.float32)], np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3))
    m.commit(0.1)
    m_ctx.setInputSource(src)
    p3 = _odo(reg_mod, 1.0, 2.0)
    p3.setInputTarget(m.target()[:, :3].copy()); p3.setInputSource(src)
    assert same(solve(m_ctx, I4), solve(p3, I4)), "map-bound"
    p3.close(); m_ctx.close()


def test_determinism_and_device_inputs(reg_mod):
    tgt, src = CL["tgt"], CL["src"]
    I4 = np.eye(4, dtype=np.float32)
    runs = []
    for kind in ("host", "host", "device"):
        for general in (False, True):
            v = _odo(reg_mod, 1.0, 2.0, reg=reg_mod.FastVGICP.REG_MIN_EIG if general else None)
            if kind == "device":
                bufs = []
                for cloud, setter in ((tgt, v.setInputTargetDevice), (src, v.setInputSourceDevice)):
                    a = np.zeros((len(cloud), 4), np.float32); a[:, :3] = cloud
                    d = v.device_alloc(a.nbytes)
                    v.upload(d, a)
                    setter(d, len(cloud), 16)
                    bufs.append(d)
            else:
                v.setInputTarget(tgt); v.setInputSource(src)
            cost, H, b = v.linearize(CL["T_lin"])
            e = v.compute_error(CL["T_err"])
            v.align(I4, want_output=False)
            runs.append((kind, general, cost, H.copy(), b.copy(), e, v.num_correspondences, v.getFinalTransformation().copy(), v.getFinalHessian().copy(),
                         v.nr_iterations))
            if kind == "device":
                for d in bufs:
                    v.device_free(d)
            v.close()
    for general in (False, True):
        a, b, c = [r for r in runs if r[1] == general]
        for other in (b, c):
            assert a[2] == other[2] and np.array_equal(a[3], other[3]) and np.array_equal(a[4], other[4]) and a[5] == other[5], (general, other[0])
            assert a[6] == other[6] and np.array_equal(a[7], other[7]) and np.array_equal(a[8], other[8]) and a[9] == other[9], (general, other[0])


def test_cpp_adaptor(reg_mod, tmp_path):
    """rgc::FastVGICPHip::setNeighborSearchMethod(DIRECT_RADIUS, 2.0): the linearisation and the solve of the Python adaptor bit for bit, a refused
    radius remembered and pending, the stored radius kept under another method"""
    exe = str(tmp_path / "test_vgicp_radius")
    subprocess.check_call(["g++", "-std=c++14", "-O2", os.path.join(ROOT, "tests", "cpp", "test_vgicp_radius.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "rgc-slam_amd"), "-lrgc_hip", "-Wl,-rpath," + os.path.join(ROOT, "rgc-slam_amd")])
    for name in ("tgt", "src"):
        with open(tmp_path / (name + ".bin"), "wb") as f:
            f.write(np.int32(len(CL[name])).tobytes())
            f.write(np.ascontiguousarray(CL[name], np.float32).tobytes())
    out = subprocess.run([exe, str(tmp_path / "tgt.bin"), str(tmp_path / "src.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "EXCEPTION" not in out.stdout, out.stdout + out.stderr
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines() if l.strip()}
    v = _odo(reg_mod, 1.0, 2.0)
    v.setInputTarget(CL["tgt"]); v.setInputSource(CL["src"])
    cost, H, b = v.linearize(np.eye(4))
    lin = np.array(lines["lin"], np.float64)
    assert lin[0] == cost and np.array_equal(lin[1:37], H.reshape(36)) and np.array_equal(lin[37:], b)
    v.align(np.eye(4, dtype=np.float32), want_output=False)
    assert np.array_equal(np.array(lines["T"], np.float32), v.getFinalTransformation().reshape(16))
    assert lines["converged"] == ["1", "iterations", str(v.nr_iterations)]
    assert lines["setters"] == ["9"], out.stdout
    v.close()
