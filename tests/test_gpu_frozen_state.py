"""What drops a frozen linearisation, on the MI355X: VGICP (rgc_linearize), FastGICP (rgc_gicp_*), FastGICPSingleThread (rgc_gicpst_*) and
FastGICPMultiPoints (rgc_gicpmp_*) each freeze per-point state on ONE context's clouds, and every call that changes those clouds, their covariances
or the settings they were prepared under must drop all four (rgcapi::drop_frozen, csrc/rgc_ctx.h): a read-out that went on afterwards would index
into clouds that are no longer there.

One context on a small two-wall scene (a target of 256 points, a source of 128, k = 10).  For every dropping call: the four methods are linearised,
the call is made, every frozen read-out (compute_error, num_correspondences, correspondences, num_searched, merged) must be refused with the status
the library has always given, and after the clouds are set and linearised again the read-outs must give what they gave before.

The statuses are the code's: the GICP family reports RGC_ERR_INVALID whether its state fell or a cloud is missing; VGICP's rgc_compute_error reports
RGC_ERR_NO_INPUT when the call left a cloud unprepared (need_inputs comes first) and RGC_ERR_INVALID when both clouds stand and only the frozen list
fell; rgc_num_correspondences is RGC_ERR_INVALID either way.  The costs after the second linearisation are compared to 1e-9 of the value: the same
fp64 terms over at most 128 points, whose summation order may differ with the grid the clouds are sorted on (at most 128 * 2^-53 = 1.4e-14)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 10
T0 = np.eye(4)
T1 = np.eye(4)
T1[:3, 3] = (0.01, -0.02, 0.005)


@pytest.fixture(scope="module")
def mod():
    from rgc_slam_amd import _lib, gicp, local_map, registration
    return dict(lib=_lib, gicp=gicp, reg=registration, map=local_map)


@pytest.fixture(scope="module")
def scene():
    """two walls meeting in a corner (x = 10 and y = -6, 4 m x 3 m each, 1 cm of noise): a target of 256 points, a source of 128 seen 5 cm away"""
    rng = np.random.default_rng(2317)

    def walls(n):
        u, h, on_x = rng.uniform(0.0, 4.0, n), rng.uniform(0.0, 3.0, n), rng.integers(0, 2, n).astype(bool)
        p = np.where(on_x[:, None], np.stack([np.full(n, 10.0), -6.0 + u, h], 1), np.stack([10.0 + u, np.full(n, -6.0), h], 1))
        return p + rng.normal(0.0, 0.01, p.shape)

    tgt = walls(256).astype(np.float32)
    src = (walls(128) + (0.05, -0.03, 0.02)).astype(np.float32)
    return dict(tgt=tgt, src=src)


@pytest.fixture(scope="module")
def ctx(mod):
    g = mod["gicp"].FastGICPSingleThread(0)
    yield g
    g.close()


def _linearize_all(mod, g):
    """the four methods linearised at T0 on the context's clouds"""
    G = mod["gicp"]
    mod["reg"].FastVGICP.linearize(g, T0)
    G.FastGICP.linearize(g, T0)
    g.linearize(T0)
    G.FastGICPMultiPoints.linearize(g, T0)


def _readouts(mod, g):
    """every frozen read-out by name: (call, the status VGICP's differs by) -- see the module docstring"""
    G, V = mod["gicp"], mod["reg"].FastVGICP
    return [
        ("vgicp compute_error", lambda: V.compute_error(g, T1), "vgicp"),
        ("vgicp num_correspondences", lambda: V.num_correspondences.fget(g), None),
        ("gicp compute_error", lambda: G.FastGICP.compute_error(g, T1), None),
        ("gicp num_correspondences", lambda: G.FastGICP.num_correspondences.fget(g), None),
        ("gicp correspondences", lambda: G.FastGICP.correspondences(g), None),
        ("gicpst compute_error", lambda: g.compute_error(T1), None),
        ("gicpst num_correspondences", lambda: g.num_correspondences, None),
        ("gicpst num_searched", lambda: g.num_searched(), None),
        ("gicpst correspondences", lambda: g.correspondences(), None),
        ("gicpmp num_correspondences", lambda: G.FastGICPMultiPoints._counts(g), None),
        ("gicpmp merged", lambda: G.FastGICPMultiPoints.merged(g), None),
    ]


def _values(mod, g):
    """the scalar read-outs, for the comparison before / after"""
    G, V = mod["gicp"], mod["reg"].FastVGICP
    out = dict(costs=(V.compute_error(g, T1), G.FastGICP.compute_error(g, T1), g.compute_error(T1)),
               counts=(V.num_correspondences.fget(g), G.FastGICP.num_correspondences.fget(g), g.num_correspondences, g.num_searched(),
                       G.FastGICPMultiPoints._counts(g)))
    idx, sq = G.FastGICP.correspondences(g)
    sidx = g.correspondences()[0]
    cnt = G.FastGICPMultiPoints.merged(g)[0]
    assert len(idx) == len(sidx) == len(cnt) == g._n_src and (idx >= 0).sum() == out["counts"][1] and (sidx >= 0).sum() == out["counts"][2]
    assert (cnt > 0).sum() == out["counts"][4][0] and int(cnt.sum()) == out["counts"][4][1]
    return out


def _standard(mod, g, scene):
    """the context back on the standard settings and the scene's clouds, the four methods linearised; returns the read-outs' values"""
    V = mod["reg"].FastVGICP
    mod["map"].RollingLocalMap(g).reset()
    g.setKernelWidth(0.5, 3.0)
    g.setNearestNeighborSearchMethod(V.NearestNeighborMethod.GPU_BRUTEFORCE)
    g.setRegularizationMethod(V.REG_PLANE)
    g.setVoxelAccumulationMode(V.VOXEL_ADDITIVE)
    g.setCorrespondenceRandomness(K)
    g.setInputTarget(scene["tgt"])
    g.setInputSource(scene["src"])
    _linearize_all(mod, g)
    return _values(mod, g)


def _assert_refused(mod, g, vgicp_status, label):
    L = mod["lib"]
    for name, call, which in _readouts(mod, g):
        want = vgicp_status if which == "vgicp" else L.ERR_INVALID
        with pytest.raises(L.RgcError) as e:
            call()
        assert e.value.status == want, (label, name, e.value.status, want, str(e.value))


def _map_bound(mod, g, scene):
    """the context's target = the committed rolling map of one keyframe (the scene's target), the four methods linearised on it"""
    m = mod["map"].RollingLocalMap(g)
    kf = np.zeros((len(scene["tgt"]), 4), np.float32)
    kf[:, :3] = scene["tgt"]
    m.reset()
    m.insert(kf, (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))
    assert m.commit(0.02) >= K
    g.setInputSource(scene["src"])
    _linearize_all(mod, g)
    _values(mod, g)
    return m, kf


# (name, NO_INPUT: the call leaves a cloud unprepared / INVALID: both clouds stand, only the frozen state fell)
CASES = [("set_params_k", "INVALID"), ("regularization_method", "NO_INPUT"), ("covariance_estimation", "NO_INPUT"), ("rbf_kernel", "NO_INPUT"),
         ("voxel_accumulation_mode", "NO_INPUT"), ("share_target", "INVALID"), ("set_source", "INVALID"), ("set_target", "INVALID"),
         ("clear_source", "NO_INPUT"), ("clear_target", "NO_INPUT"), ("swap", "INVALID"), ("source_covariances", "INVALID"),
         ("target_covariances", "INVALID"), ("map_reset", "NO_INPUT"), ("map_rebase", "NO_INPUT"), ("map_commit", "INVALID")]


@pytest.mark.parametrize("name,left", CASES, ids=[c[0] for c in CASES])
def test_dropping_call_refuses_every_frozen_readout(mod, ctx, scene, name, left):
    L, V, g = mod["lib"], mod["reg"].FastVGICP, ctx
    before = _standard(mod, g, scene)
    owner = None
    if name == "set_params_k":
        g.setCorrespondenceRandomness(K + 2)
    elif name == "regularization_method":
        g.setRegularizationMethod(V.REG_FROBENIUS)
    elif name == "covariance_estimation":
        g.setNearestNeighborSearchMethod(V.NearestNeighborMethod.GPU_RBF_KERNEL)
    elif name == "rbf_kernel":  # (the kernel matters under RGC_COV_RBF only: the clouds set and linearised under it first)
        g.setNearestNeighborSearchMethod(V.NearestNeighborMethod.GPU_RBF_KERNEL)
        g.setInputTarget(scene["tgt"])
        g.setInputSource(scene["src"])
        _linearize_all(mod, g)
        _values(mod, g)
        g.setKernelWidth(0.6, 3.0)
    elif name == "voxel_accumulation_mode":
        g.setVoxelAccumulationMode(V.VOXEL_MULTIPLICATIVE)
    elif name == "share_target":
        owner = V(0)
        owner.setCorrespondenceRandomness(K)
        owner.setInputTarget(scene["tgt"])
        g.shareTargetFrom(owner)
    elif name == "set_source":
        g.setInputSource(scene["src"])
    elif name == "set_target":
        g.setInputTarget(scene["tgt"])
    elif name == "clear_source":
        g.clearSource()
    elif name == "clear_target":
        g.clearTarget()
    elif name == "swap":
        g.swapSourceAndTarget()
    elif name == "source_covariances":
        g.setSourceCovariances(g.getSourceCovariances())
    elif name == "target_covariances":
        g.setTargetCovariances(g.getTargetCovariances())
    elif name == "map_reset":
        _map_bound(mod, g, scene)[0].reset()
    elif name == "map_rebase":
        _map_bound(mod, g, scene)[0].rebase((1.0, 0.0, 0.0))
    elif name == "map_commit":
        m, kf = _map_bound(mod, g, scene)
        m.insert(kf + np.float32(0.005), (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))
        assert m.commit(0.02) >= K
    _assert_refused(mod, g, getattr(L, "ERR_" + left), name)
    try:
        after = _standard(mod, g, scene)
    finally:
        if owner is not None:
            owner.close()
    assert after["counts"] == before["counts"], (name, before, after)
    assert after["costs"] == pytest.approx(before["costs"], rel=1e-9), (name, before, after)
