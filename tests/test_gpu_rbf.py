"""RBF-kernel covariance estimation on the GPU (rgc_set_covariance_estimation(RGC_COV_RBF), k_rbf_cov6 in csrc/rgc_rbf.hip) against tests/rbf_reference.py.

NONE is held to the derived bar |gpu - ref| <= (m + 8) u sum|terms| / S0 per entry (rbf_reference's module text has the derivation), the eigen-based
regularisations to the same bound matrix propagated as 4 max(value) ||B||_F / gap on the rows whose gap is at least 1e-6 of the trace, FROBENIUS to B scaled
by the condition number of S + 1e-3 I.  Each test prints the largest observed ratio to its bar before it asserts.  The cases (tests/rbf_cases.py): the
dyadic lattice at three cell sizes (members exactly on the radius, reach 3 / 2 / 1 cells), the knife-edge pairs, max_dist < res, max_dist larger than the
cloud, corner cells, a cell with more points than a candidate tile and a workgroup's run, n = 1, 2, 63, 64, 65, an isolated point, a jittered wall-and-floor
scene at the defaults under all five methods; then the data paths and the plumbing bit for bit, and the setters.
Largest ratio to the NONE bar observed on one MI355X: 0.097 ("short"), 0.053 ("crowded"); the eigen-based methods 0.027 at most (EXPERIMENTS.md "10a").
"""
import ctypes as C

import numpy as np
import pytest

import rbf_cases as rc
import rbf_reference as rr

pytestmark = pytest.mark.gpu

NONE, MIN_EIG, NORMALIZED_MIN_EIG, PLANE, FROBENIUS = range(5)
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def reg_mod():
    from rgc_slam_amd import registration
    return registration


def _rbf(reg_mod, kw, md, res=1.0, method=NONE):
    v = reg_mod.FastVGICP(0)
    v.setResolution(res)
    v.setRegularizationMethod(method)
    v.setNearestNeighborSearchMethod(v.NearestNeighborMethod.GPU_RBF_KERNEL)
    v.setKernelWidth(kw, md)
    return v


def _target_cov(reg_mod, name, method=NONE):
    P, kw, md, res = rc.case(name)
    v = _rbf(reg_mod, kw, md, res, method)
    v.setInputTarget(P)
    got = v.getTargetCovariances()
    v.close()
    return got


def _check(got, name, method):
    m = rc.mom(name)
    exp = rr.regularize(m["cov"], rr.METHODS[method])
    B, ok = rr.bound(m, rr.METHODS[method])
    assert (~ok).mean() <= 0.05
    assert np.all(np.isfinite(got)) and np.all(got == np.transpose(got, (0, 2, 1)))
    err = np.abs(got - exp)[ok]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err == 0, 0.0, err / np.broadcast_to(B, got.shape)[ok])
    print(f"rbf {name} {rr.METHODS[method]}: rows {int(ok.sum())}/{len(ok)} mean ball {m['m'].mean():.1f} largest |gpu - ref| / bar = {ratio.max(initial=0.0):.4f}")
    assert np.all(err <= np.broadcast_to(B, got.shape)[ok]), float(ratio.max())


@pytest.mark.parametrize("name", rc.NONE_CASES)
def test_none_against_the_reference(reg_mod, name):
    _check(_target_cov(reg_mod, name), name, NONE)


@pytest.mark.parametrize("method", [MIN_EIG, NORMALIZED_MIN_EIG, PLANE, FROBENIUS])
@pytest.mark.parametrize("name", rc.EIGEN_CASES)
def test_regularisations_against_the_reference(reg_mod, name, method):
    _check(_target_cov(reg_mod, name, method), name, method)


def test_lattice_agrees_across_cell_sizes(reg_mod):
    """The cell size sets the cloud's sorted order, and with it the order a ball is summed in: the three results are three roundings of the same sums, so
    they differ from each other by at most twice the bar each is held to (and may differ in the last bits).  What does NOT change the order -- the grid's
    extent, the spans the candidates come from -- leaves the bits alone: test_host_device_and_repeated_runs_are_bit_identical prepares the same cloud on
    a measured and on a speculative (wider) grid of the same cell size."""
    a, b, c = (_target_cov(reg_mod, "lattice_" + r) for r in ("0.5", "1", "2"))
    B = rr.bound_none(rc.mom("lattice_1"))
    for x, y in ((a, b), (a, c), (b, c)):
        d = np.abs(x - y)
        print(f"rbf lattice pair: largest difference / (2 bar) = {np.max(d / (2 * B)):.4f}")
        assert np.all(d <= 2 * B)


def test_isolated_point_under_every_method(reg_mod):
    i = rc.ISOLATED_ROW
    assert np.all(_target_cov(reg_mod, "isolated", NONE)[i] == 0)
    assert np.allclose(_target_cov(reg_mod, "isolated", MIN_EIG)[i], 1e-3 * np.eye(3), rtol=0, atol=1e-18)
    assert np.allclose(_target_cov(reg_mod, "isolated", NORMALIZED_MIN_EIG)[i], 1e-3 * np.eye(3), rtol=0, atol=1e-18)
    assert np.allclose(np.linalg.eigvalsh(_target_cov(reg_mod, "isolated", PLANE)[i]), [1e-3, 1, 1], rtol=0, atol=1e-15)   # (a zero moment has no normal: any basis)
    assert np.allclose(_target_cov(reg_mod, "isolated", FROBENIUS)[i], np.sqrt(3.0) * np.eye(3), rtol=1e-14, atol=0)


def test_source_on_its_own_grid(reg_mod):
    for name in ("scene_src", "knife", "crowded", "tiny_1"):
        P, kw, md, res = rc.case(name)
        v = _rbf(reg_mod, kw, md, res)
        v.setInputSource(P)
        got = v.getSourceCovariances()
        v.close()
        _check(got, name, NONE)


def test_host_device_and_repeated_runs_are_bit_identical(reg_mod):
    P, kw, md, res = rc.case("scene")
    v = _rbf(reg_mod, kw, md, res, MIN_EIG)
    v.setInputTarget(P); v.setInputSource(P[::3].copy())
    t0, s0 = v.getTargetCovariances(), v.getSourceCovariances()
    v.setInputTarget(P); v.setInputSource(P[::3].copy())
    assert np.array_equal(t0, v.getTargetCovariances()) and np.array_equal(s0, v.getSourceCovariances())
    P4 = np.zeros((len(P), 4), np.float32); P4[:, :3] = P
    S4 = np.ascontiguousarray(P4[::3])
    dt, ds = v.device_alloc(P4.nbytes), v.device_alloc(S4.nbytes)
    v.upload(dt, P4); v.upload(ds, S4)
    v.setInputTargetDevice(dt, len(P4), 16); v.setInputSourceDevice(ds, len(S4), 16)
    assert np.array_equal(t0, v.getTargetCovariances()) and np.array_equal(s0, v.getSourceCovariances())
    w = _rbf(reg_mod, kw, md, res, MIN_EIG)                                  # ... and on another context
    w.setInputTarget(P)
    assert np.array_equal(t0, w.getTargetCovariances())
    w.close()
    v.device_free(dt); v.device_free(ds)
    v.close()


def test_reframed_and_swapped_targets(reg_mod):
    P, kw, md, res = rc.case("scene")
    v = _rbf(reg_mod, kw, md, res)
    P4 = np.zeros((len(P), 4), np.float32); P4[:, :3] = P
    d_map, d_scr = v.device_alloc(P4.nbytes), v.device_alloc(P4.nbytes)
    v.upload(d_map, P4)
    q = np.array([0.0, 0.0, np.sin(0.05), np.cos(0.05)]); t = np.array([1.5, -2.25, 0.125])
    v.setInputTargetReframed(d_map, len(P4), 16, q, t, d_scr)
    got = v.getTargetCovariances()
    moved = v.download(d_scr, (len(P4), 4))
    w = _rbf(reg_mod, kw, md, res)
    w.setInputTarget(np.ascontiguousarray(moved[:, :3]))
    assert np.array_equal(got, w.getTargetCovariances())
    # swapped: the source becomes the target
    S = rc.case("scene_src")[0]
    v.setInputTarget(P); v.setInputSource(S)
    v.swapSourceAndTarget()
    w.setInputTarget(S); w.setInputSource(P)
    assert np.array_equal(v.getTargetCovariances(), w.getTargetCovariances()) and np.array_equal(v.getSourceCovariances(), w.getSourceCovariances())
    v.device_free(d_map); v.device_free(d_scr)
    v.close(); w.close()


def test_plumbing_bit_for_bit(reg_mod):
    """the RBF covariances read back and injected into a context on the kNN general route: every consumer returns the same bits on both"""
    P, kw, md, res = rc.case("scene")
    T = np.eye(4); T[:3, 3] = (0.04, -0.03, 0.01)
    S = (P[::2].astype(np.float64) @ T[:3, :3].T - T[:3, 3]).astype(np.float32)
    a = _rbf(reg_mod, kw, md, res)
    a.setInputTarget(P); a.setInputSource(S)
    ct, cs = a.getTargetCovariances(), a.getSourceCovariances()
    b = reg_mod.FastVGICP(0)
    b.setResolution(res); b.setRegularizationMethod(NONE)
    b.setInputTarget(P); b.setInputSource(S)
    assert not np.array_equal(ct, b.getTargetCovariances())
    b.setTargetCovariances(ct); b.setSourceCovariances(cs)
    assert np.array_equal(ct, b.getTargetCovariances()) and np.array_equal(cs, b.getSourceCovariances())
    res_ = []
    for v in (a, b):
        cost, H, g = v.linearize(np.eye(4))
        cg, Hg, gg = C.c_double(0), np.empty(36), np.empty(6)
        Tg = np.eye(4).reshape(16)
        v._chk(v._L.rgc_gicp_linearize(v._h, Tg.ctypes.data_as(DP), Hg.ctypes.data_as(DP), gg.ctypes.data_as(DP), C.byref(cg)))
        v.align(np.eye(4, dtype=np.float32), want_output=False)
        res_.append((cost, H, g, cg.value, Hg.copy(), gg.copy(), v.getFinalTransformation().copy(), v.getFinalHessian().copy()))
    for x, y in zip(*res_):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    a.close(); b.close()


def _get(v):
    m, kw, md = C.c_int(-1), C.c_double(0), C.c_double(0)
    v._chk(v._L.rgc_get_covariance_estimation(v._h, C.byref(m)))
    v._chk(v._L.rgc_get_rbf_kernel(v._h, C.byref(kw), C.byref(md)))
    return m.value, kw.value, md.value


def test_setters(reg_mod):
    P, _, _, _ = rc.case("corners")
    v = reg_mod.FastVGICP(0)
    L, h = v._L, v._h
    assert _get(v) == (0, 0.5, 3.0)                                          # defaults: kNN, fast_vgicp_cuda_impl.hpp:31
    v.setInputTarget(P)
    tuned = v.getTargetCovariances()
    # refused, the context intact
    for kw, md in ((0.0, 0.0), (-1.0, 3.0), (float("nan"), 3.0), (float("inf"), 3.0), (1e300, 3.0), (0.5, float("nan"))):
        assert L.rgc_set_rbf_kernel(h, kw, md) == -1 and _get(v) == (0, 0.5, 3.0)
    for m in (-1, 2, 99):
        assert L.rgc_set_covariance_estimation(h, m) == -1 and _get(v) == (0, 0.5, 3.0)
    assert L.rgc_get_covariance_estimation(h, None) == -1 and L.rgc_get_rbf_kernel(h, None, None) == -1
    assert np.array_equal(tuned, v.getTargetCovariances())
    # no-ops keep the clouds: the current method again; the kernel while kNN is selected
    assert L.rgc_set_covariance_estimation(h, 0) == 0 and L.rgc_set_rbf_kernel(h, 0.25, -1.0) == 0
    assert _get(v) == (0, 0.25, 1.25)                                        # max_dist <= 0: 5 * kernel_width
    assert L.rgc_set_rbf_kernel(h, 0.25, 0.0) == 0 and _get(v) == (0, 0.25, 1.25)
    assert np.array_equal(tuned, v.getTargetCovariances())
    # a change drops them
    v.setNearestNeighborSearchMethod(v.NearestNeighborMethod.GPU_RBF_KERNEL)
    assert _get(v)[0] == 1
    with pytest.raises(reg_mod.RgcError):
        v.getTargetCovariances()
    v.setInputTarget(P)
    rbf = v.getTargetCovariances()
    assert not np.array_equal(rbf, tuned)
    v.setKernelWidth(0.25, 1.25)                                             # the current kernel again: kept
    v.setNearestNeighborSearchMethod(v.NearestNeighborMethod.GPU_RBF_KERNEL)
    assert np.array_equal(rbf, v.getTargetCovariances())
    v.setKernelWidth(0.25, 1.5)                                              # another kernel under RBF: dropped
    with pytest.raises(reg_mod.RgcError):
        v.getTargetCovariances()
    v.setInputTarget(P)
    assert not np.array_equal(rbf, v.getTargetCovariances())
    # RGC_ERR_TOO_FEW_POINTS does not apply under RBF; it does again under kNN
    v.setInputTarget(P[:1].copy())
    assert v.getTargetCovariances().shape == (1, 3, 3)
    for m in (v.NearestNeighborMethod.GPU_BRUTEFORCE, v.NearestNeighborMethod.GPU_RBF_KERNEL, v.NearestNeighborMethod.CPU_PARALLEL_KDTREE):
        v.setNearestNeighborSearchMethod(m)
    assert _get(v)[0] == 0
    with pytest.raises(reg_mod.RgcError) as e:
        v.setInputTarget(P[:1].copy())
    assert e.value.status == -3
    with pytest.raises(ValueError):
        v.setNearestNeighborSearchMethod(3)
    # kNN after RBF: the tuned route's bits
    v.setInputTarget(P)
    assert np.array_equal(tuned, v.getTargetCovariances())
    v.close()
