"""The scan front-end (A1-A8) on the designed sweeps of tests/fe_cases.py, each run three ways: through the host-pointer call, on a
second context through the speculative path (cloud=False: launches sized from the previous sweep), and through laserCloudHandlerMsg on
message bytes.  Every result is held to the C oracle by test_gpu_frontend._compare, unchanged, with time_outliers = 0; the
speculative results must equal the synchronous ones array for array.

PROOF OF ROUTE: the library has no read-out of the selection's staging group or of the speculative path's fall-back, so the route is
proven from the reference alone -- tests/test_fe_cases.py asserts, without a GPU, that each sweep makes the reference take the branch
the case is named for (ties that decide a pick, quota cuts, sectors that differ from their run in isolation, the largest ring against
the launcher's switch points written down in fe_cases.STAGING).  -m gpu."""
import types

import numpy as np
import pytest

import fe_cases
from test_gpu_frontend import _compare

pytestmark = pytest.mark.gpu

KEYS = ("curvature", "curvature2", "inten_curvature", "ground_marked", "picked", "label", "inten_label", "sharp", "flat", "inten", "ground_pts")
ACCEPTED = [n for n, c in fe_cases.CASES.items() if not c.refused]
REFUSED = [n for n, c in fe_cases.CASES.items() if c.refused]


class _Ctx:
    """one library context, its parameters set per sweep"""
    def __init__(self):
        from rgc_slam_amd import frontend
        self.fe = frontend.ScanRegistration(16)

    def on(self, prm):
        self.fe.params.n_scans, self.fe.params.use_intensity = prm["n_scans"], prm.get("use_intensity", 1)
        return self.fe


@pytest.fixture(scope="module")
def ctx():
    c = {k: _Ctx() for k in ("host", "spec", "msg")}
    yield c
    for v in c.values():
        v.fe.close()


_sync = {}


def _oracle(orc, prm):
    return types.SimpleNamespace(frontend=lambda raw, n_scans: orc.frontend(raw, **prm))


def _host(ctx, orc, name):
    """the host-pointer call on a case against the oracle (once per case: the speculative tests compare with it)"""
    if name not in _sync:
        raw, prm, _ = fe_cases.get(name)
        _sync[name] = _compare(ctx["host"].on(prm), _oracle(orc, prm), raw, prm["n_scans"], time_outliers=0)
    return _sync[name]


def _same(a, b):
    assert a["n_cloud"] == b["n_cloud"] and np.array_equal(a["ring_count"], b["ring_count"])
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert a["n_sharp_own"] == b["n_sharp_own"] and a["n_ground"] == b["n_ground"] and a["ground_valid"] == b["ground_valid"]
    assert np.array_equal(a["groundparam"], b["groundparam"])


@pytest.mark.parametrize("name", ACCEPTED)
def test_host_pointer(ctx, orc, name):
    g, o = _host(ctx, orc, name)
    assert g["n_cloud"] == o["n_cloud"]


@pytest.mark.parametrize("name", ACCEPTED)
def test_speculative_after_itself(ctx, orc, name):
    """the case twice on the second context with the sweep left on the device: the second run is sized from the first (for a largest
    ring of 2555 .. 3256 the guess `prev + prev / 4 + 64` crosses a staging switch: three sectors per window where the synchronous path
    stages six; likewise below the other two switches).  That the second run is speculative, and with which window, is derived from the
    ring counts by tests/test_fe_cases.py::test_speculative_sequence_routes -- this test cannot see it."""
    raw, prm, _ = fe_cases.get(name)
    g, _ = _host(ctx, orc, name)
    fe = ctx["spec"].on(prm)
    for _ in range(2):
        _same(fe.laserCloudHandler(raw, cloud=False), g)


@pytest.mark.parametrize("name", ACCEPTED)
def test_message_bytes(ctx, orc, name):
    from rgc_slam_amd import wire
    raw, prm, _ = fe_cases.get(name)
    m = np.zeros((len(raw), 8), np.float32)
    m[:, :3] = raw[:, :3]
    m[:, 4] = raw[:, 3]
    lay = wire.layout(32, dict(x=(0, 7), y=(4, 7), z=(8, 7), intensity=(16, 7)))
    fe = ctx["msg"].on(prm)
    via = types.SimpleNamespace(laserCloudHandler=lambda r: fe.laserCloudHandlerMsg(m.tobytes(), len(r), lay))
    g, _ = _compare(via, _oracle(orc, prm), raw, prm["n_scans"], time_outliers=0)
    _same(g, _host(ctx, orc, name)[0])


def _refused(fe, raw, **kw):
    from rgc_slam_amd import _lib
    with pytest.raises(_lib.RgcError) as e:
        fe.laserCloudHandler(raw, **kw)
    assert e.value.status == _lib.ERR_INVALID and "a ring sector holds more than 2048 points" in str(e.value)


def test_speculative_sequence(ctx, orc):
    """fe_cases.SPEC_SEQUENCE on one context, every sweep left on the device: the largest ring the window guessed from the previous sweep
    holds (guess + 12) and the first it does not (guess + 13: done again), an empty sweep in between, fewer sectors per window than
    the synchronous path, a change of n_scans, the oversize sweep arriving on the speculative path (refused; the sweeps after it are
    right).  The routes are asserted from the ring counts in tests/test_fe_cases.py::test_speculative_sequence_routes."""
    spec = ctx["spec"]
    spec.on(dict(n_scans=16)).laserCloudHandler(fe_cases.get("spec_1000")[0], cloud=False)
    for step, route, _ in fe_cases.SPEC_SEQUENCE:
        name = step.split("@")[0]
        raw, prm, _ = fe_cases.get(name)
        assert prm["n_scans"] == int(step.split("@")[1]) if "@" in step else prm["n_scans"] == 16
        if fe_cases.CASES[name].refused:
            assert route == "refused"
            _refused(spec.on(prm), raw, cloud=False)
            continue
        if name == "empty":
            a = spec.on(prm).laserCloudHandler(raw, cloud=False)
            assert a["n_cloud"] == 0 and len(a["sharp"]) == 0 and not a["ground_valid"]
            continue
        _same(spec.on(prm).laserCloudHandler(raw, cloud=False), _host(ctx, orc, name)[0])


@pytest.mark.parametrize("name", REFUSED)
def test_oversize_sector_is_refused(ctx, orc, name):
    """a sector of 2049 points: RGC_ERR_INVALID with its message from the host-pointer call, from the speculative path and from message
    bytes (the device-pointer entry); the next sweep on each context is right"""
    raw, prm, _ = fe_cases.get(name)
    after = "ring_12298"
    g, _ = _host(ctx, orc, after)
    _refused(ctx["host"].on(prm), raw)
    _sync.pop(after)
    _same(_host(ctx, orc, after)[0], g)                                  # the same context, against the oracle again
    spec = ctx["spec"].on(prm)
    _same(spec.laserCloudHandler(fe_cases.get(after)[0], cloud=False), g)
    _refused(spec, raw, cloud=False)                                      # sized from the sweep before it: refused on the speculative path
    for _ in range(2):
        _same(spec.laserCloudHandler(fe_cases.get(after)[0], cloud=False), g)
    from rgc_slam_amd import _lib, wire
    lay = wire.layout(32, dict(x=(0, 7), y=(4, 7), z=(8, 7), intensity=(16, 7)))
    msg = ctx["msg"].on(prm)

    def packed(a):
        m = np.zeros((len(a), 8), np.float32)
        m[:, :3], m[:, 4] = a[:, :3], a[:, 3]
        return m.tobytes()
    with pytest.raises(_lib.RgcError) as e:
        msg.laserCloudHandlerMsg(packed(raw), len(raw), lay)
    assert e.value.status == _lib.ERR_INVALID and "a ring sector holds more than 2048 points" in str(e.value)
    ok = fe_cases.get(after)[0]
    _same(msg.laserCloudHandlerMsg(packed(ok), len(ok), lay), g)
