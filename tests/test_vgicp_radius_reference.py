"""The offset table of VGICP's DIRECT_RADIUS method (rgc_neighbor_offsets: host code, no context) against tests/vgicp_radius_reference.py, which
restates src/fast_gicp/cuda/fast_vgicp_cuda.cu:77-91 in numpy:

  * the table offset for offset and in order at every radius where its size changes (1, 7, 19, 27, 33, 57, 123, 485 offsets), and the tables of
    DIRECT27 / DIRECT7 / DIRECT1 against vgicp_reference.OFFSETS;
  * its shape: at 1.7311 it IS DIRECT27's list, at 1.0 DIRECT7's as a set in another order;
  * refusals: a radius of 5.0 (515 offsets, above RGC_NDT_MAX_OFFSETS), NaN, inf and a negative radius under method 3, a method outside 0..3, a
    NULL n; methods 0..2 take any radius; a cap below the table writes cap offsets and reports the total;
  * the wiring of the numpy reference: a linearisation over the 1.7311 table equals the one over "DIRECT27" bit for bit.

No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import vgicp_radius_reference as vrr
import vgicp_reference as vr


@pytest.fixture(scope="module")
def L():
    from rgc_slam_amd import _lib
    return _lib.load()


def _table(L, method, radius, cap=None):
    n = C.c_int(-1)
    rc = L.rgc_neighbor_offsets(method, radius, None, 0, C.byref(n))
    if rc != 0:
        return rc, None, None
    cap = n.value if cap is None else cap
    buf = np.full((max(cap, 1) + 2, 3), 77, np.int32)               # two guard rows behind the capacity
    rc = L.rgc_neighbor_offsets(method, radius, buf.ctypes.data_as(C.POINTER(C.c_int)), cap, C.byref(n))
    assert np.all(buf[cap:] == 77), "wrote past cap"
    return rc, n.value, buf[:min(cap, n.value)].astype(np.int64)


@pytest.mark.parametrize("radius,count", sorted(vrr.COUNTS.items()))
def test_table_counts_and_order(L, radius, count):
    ref = vrr.offsets(radius)
    assert len(ref) == count, (radius, len(ref))                     # the helper against the counts worked out from the rule
    rc, n, got = _table(L, vrr.DIRECT_RADIUS, radius)
    assert rc == 0 and n == count, (radius, rc, n)
    assert np.array_equal(got, ref), radius


def test_fixed_methods_and_python_adaptor(L):
    from rgc_slam_amd import _lib, registration
    assert (_lib.DIRECT27, _lib.DIRECT7, _lib.DIRECT1, _lib.DIRECT_RADIUS) == (0, 1, 2, 3)
    assert registration.NeighborSearchMethod.DIRECT_RADIUS == 3
    for code, name in enumerate(vr.METHODS):
        for radius in (-1.0, 0.0, 2.0, 100.0, math.nan, math.inf):   # ignored, whatever it is
            rc, n, got = _table(L, code, radius)
            assert rc == 0 and np.array_equal(got, vr.OFFSETS[name]), (name, radius)
    assert np.array_equal(registration.FastVGICP.neighbor_offsets(3, 2.0), vrr.offsets(2.0))
    assert np.array_equal(registration.FastVGICP.neighbor_offsets(1), vr.OFFSETS["DIRECT7"])
    with pytest.raises(registration.RgcError):
        registration.FastVGICP.neighbor_offsets(3, 5.0)


def test_table_shape(L):
    _, _, t27 = _table(L, 3, 1.7311)
    assert np.array_equal(t27, vr.OFFSETS["DIRECT27"])               # the same list in the same order
    _, _, t7 = _table(L, 3, 1.0)
    d7 = vr.OFFSETS["DIRECT7"]
    assert sorted(map(tuple, t7)) == sorted(map(tuple, d7)) and not np.array_equal(t7, d7)
    _, _, t1 = _table(L, 3, 0.0)
    assert np.array_equal(t1, vr.OFFSETS["DIRECT1"])


def test_refusals(L):
    n = C.c_int(-5)
    assert len(vrr.offsets(5.0)) == 515 > vrr.MAX_OFFSETS
    for radius in (5.0, math.nan, math.inf, -math.inf, -0.5, 1.0e9):
        assert L.rgc_neighbor_offsets(3, radius, None, 0, C.byref(n)) == -1 and n.value == -5, radius
    for m in (-1, 4, 99):
        assert L.rgc_neighbor_offsets(m, 1.0, None, 0, C.byref(n)) == -1 and n.value == -5, m
    assert L.rgc_neighbor_offsets(3, 1.0, None, 0, None) == -1       # NULL n
    assert L.rgc_neighbor_offsets(3, 1.0, None, -1, C.byref(n)) == -1
    rc, total, got = _table(L, 3, 3.0, cap=10)                       # a short buffer: cap offsets written, the total reported
    assert rc == 0 and total == 123 and np.array_equal(got, vrr.offsets(3.0)[:10])
    rc, total, got = _table(L, 3, 4.9)
    assert rc == 0 and total == 485 <= vrr.MAX_OFFSETS


def test_reference_wiring_equals_direct27_bit_for_bit():
    rng = np.random.default_rng(12)
    tgt = rng.uniform(-6.0, 6.0, (3000, 3)).astype(np.float32)
    src = rng.uniform(-5.0, 5.0, (700, 3)).astype(np.float32)

    def covs(n):
        A = rng.normal(size=(n, 3, 3))
        return np.einsum("nij,nkj->nik", A, A) + 0.05 * np.eye(3)

    ct, cs = covs(len(tgt)), covs(len(src))
    from scipy.spatial.transform import Rotation
    T = np.eye(4); T[:3, :3] = Rotation.from_rotvec([0.02, -0.03, 0.05]).as_matrix(); T[:3, 3] = [0.3, -0.2, 0.1]
    T2 = T.copy(); T2[:3, 3] += [0.01, 0.02, -0.01]
    for res in (0.75, 1.0):
        table = vr.voxel_table(tgt, ct, res)
        a = vr.linearize(src, cs, table, T, res, vrr.method(1.7311))
        b = vr.linearize(src, cs, table, T, res, "DIRECT27")
        assert len(a[3]["src"]) == len(b[3]["src"]) > len(src)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert np.array_equal(a[3]["src"], b[3]["src"]) and np.array_equal(a[3]["vox"], b[3]["vox"]) and np.array_equal(a[3]["M"], b[3]["M"])
        assert vr.compute_error(src, table, a[3], T2) == vr.compute_error(src, table, b[3], T2)
        n1 = len(vr.correspondences(src, cs, table, T, res, vrr.method(0.0))["src"])
        n33 = len(vr.correspondences(src, cs, table, T, res, vrr.method(2.0))["src"])
        assert n1 == len(vr.correspondences(src, cs, table, T, res, "DIRECT1")["src"]) < len(a[3]["src"]) < n33
