"""No GPU: the HOST compile of the solvers' shared Gauss-Newton term and R C R^T (csrc/rgc_terms.h: gn_term in both forms, want_H on and off, and
rcrt6; built by g++ as plain C++ with -ffp-contract=off into tests/cpp/terms_table.cpp, run once as a child process) against a numpy.longdouble
evaluation of J^T M J, J^T M e, e^T M e and R C R^T on designed rows: M identity, diagonal with a 1e6 spread, dense SPD, and the zero matrix a
singular sum becomes; q and e on an axis, tiny, and of order 100 m.

The bar is derived, not measured.  Every output is a sum of at most three products of (a sum of at most three products): at most 8 roundings along
any path, a ninth for the weight of the summing form.  So |got - ref| <= 16 * 2^-53 * (the same sum with absolute values): J^T M J against
|J|^T |M| |J|, J^T M e against |J|^T |M| |e|, the cost against |e|^T |M| |e|, R C R^T against |R| |C| |R|^T -- nearly a factor two of margin."""
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgc-slam_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "terms_table.cpp")
LD = np.longdouble
U = 16.0 * 2.0 ** -53


def _sym(m6):
    a, b, c, d, e, f = m6
    return np.array([[a, b, c], [b, d, e], [c, e, f]], dtype=np.float64)


def _rot(axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


MATS = {"identity": (1.0, 0.0, 0.0, 1.0, 0.0, 1.0),
        "diag_1e6": (1e-3, 0.0, 0.0, 1.0, 0.0, 1e3),
        "dense_spd": (4.0, 1.5, -0.75, 3.0, 0.5, 2.0),
        "zero": (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)}
QS = {"axis_x": (1.0, 0.0, 0.0), "axis_z": (0.0, 0.0, -2.5), "tiny": (3e-9, -1e-9, 2e-9), "far": (120.25, -85.5, 40.125)}
ES = {"axis_y": (0.0, 0.5, 0.0), "tiny": (-2e-9, 1e-9, 4e-9), "far": (-97.75, 110.5, -33.0)}
WS = (1.0, float(np.sqrt(7.0)), 0.3)
ROTS = (np.eye(3), _rot((0, 0, 1), np.pi / 2), _rot((1.0, -2.0, 0.5), 0.7))


def rows():
    out, names = [], []
    for k, ((mn, M), (qn, q), (en, e)) in enumerate(itertools.product(MATS.items(), QS.items(), ES.items())):
        out.append(np.concatenate([M, q, e, [WS[k % 3]], ROTS[k % 3].reshape(9), M]))
        names.append(f"{mn}/{qn}/{en}")
    return np.array(out, dtype=np.float64), names


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """(rows, names, results): one build, one child process; read only"""
    td = tmp_path_factory.mktemp("terms")
    exe, fin, fout = str(td / "terms_table"), str(td / "rows.bin"), str(td / "results.bin")
    subprocess.check_call(["g++", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-std=c++17", "-O3", "-ffp-contract=off", "-Wall",
                           "-Wno-unknown-pragmas", "-I", CSRC, SRC, "-o", exe])
    R, names = rows()
    assert R.shape == (48, 28)
    R.tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(fout, dtype=np.float64).reshape(len(R), 118)
    return R, names, got


def reference(row):
    """-> (values[28], magnitudes[28]) in longdouble: the upper triangle of J^T M J by rows, J^T M e, e^T M e, and the same with absolute values"""
    M, q, e = _sym(row[0:6]).astype(LD), row[6:9].astype(LD), row[9:12].astype(LD)
    J = np.zeros((3, 6), dtype=LD)
    J[:, :3] = np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]], dtype=LD)
    J[:, 3:] = -np.eye(3, dtype=LD)
    iu = np.triu_indices(6)
    H, b, c = J.T @ M @ J, J.T @ M @ e, e @ M @ e
    aH, ab, ac = np.abs(J).T @ np.abs(M) @ np.abs(J), np.abs(J).T @ np.abs(M) @ np.abs(e), np.abs(e) @ np.abs(M) @ np.abs(e)
    return np.concatenate([H[iu], b, [c]]), np.concatenate([aH[iu], ab, [ac]])


@pytest.mark.parametrize("form", ["sum", "set"])
def test_term_against_longdouble(table, form):
    R, names, got = table
    worst = 0.0
    for row, name, g in zip(R, names, got):
        val, mag = reference(row)
        w = LD(row[12]) if form == "sum" else LD(1.0)
        full, cost_only = (g[0:28], g[28:56]) if form == "sum" else (g[56:84], g[84:112])
        err = np.abs(full.astype(LD) - w * val)
        bar = U * abs(w) * mag
        assert (err <= bar).all(), (name, form, np.flatnonzero(err > bar))
        worst = max(worst, float(np.max(np.where(mag > 0, err / np.where(mag > 0, abs(w) * mag, 1) / 2.0 ** -53, 0.0))))
        # want_H off: the cost is the same double, nothing else is touched
        assert cost_only[27] == full[27] and not cost_only[:27].any(), name
        if name.startswith("zero/"):
            assert not full.any(), name
    print(f"{form}: worst deviation {worst:.3f} x 2^-53 of the magnitude sum (bar 16)")


def test_the_two_forms_agree_where_the_weight_is_one(table):
    """w = 1.0 and accumulators that start from +0.0: 0 + 1 * x is x, but for the sign of a zero"""
    R, _, got = table
    rows_w1 = np.flatnonzero(R[:, 12] == 1.0)
    assert len(rows_w1) == 16
    assert np.array_equal(got[rows_w1, 0:28], got[rows_w1, 56:84])


def test_rcrt_against_longdouble(table):
    R, names, got = table
    for row, name, g in zip(R, names, got):
        Rm, C = row[13:22].reshape(3, 3).astype(LD), _sym(row[22:28]).astype(LD)
        iu = np.triu_indices(3)
        val, mag = (Rm @ C @ Rm.T)[iu], (np.abs(Rm) @ np.abs(C) @ np.abs(Rm).T)[iu]
        assert (np.abs(g[112:118].astype(LD) - val) <= U * mag).all(), name


def test_what_the_rows_cover():
    R, names = rows()
    assert len(set(names)) == 48
    spread = np.abs(R[:, [0, 3, 5]])
    assert (spread.max(axis=1) / np.where(spread.min(axis=1) > 0, spread.min(axis=1), 1) >= 1e6).sum() == 12
    assert (np.abs(R[:, 6:9]).max(axis=1) > 100).sum() == 12 and (np.abs(R[:, 6:9]).max(axis=1) < 1e-8).sum() == 12
    assert (np.abs(R[:, 9:12]).max(axis=1) > 100).sum() == 16 and (np.abs(R[:, 9:12]).max(axis=1) < 1e-8).sum() == 16
