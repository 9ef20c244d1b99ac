"""Designed inputs for the scalar code of the device LM -- rgclm::so3_exp_R, solve_ldlt6, lm_try (csrc/rgc_lm.h) and rgck::lm_step_decide
(csrc/rgc_lm_decide.h) -- as the five tables tests/cpp/lm_device_table.hip evaluates with the host compile and the device compile of those functions,
the checks of each table against tests/lm_reference.py, and the bars.

The bars.  The reference arithmetic of a bar is the HOST compile (closed form, true division): HOST_FIGURES holds the host's largest deviation from
the longdouble reference per class of check, in units of u = 2^-53, measured on the tables below by

    python tests/lm_cases.py            (builds the host half into a temporary directory, prints every figure)

and rounded up to two digits.  tests/test_lm_reference.py holds the host to those figures (so they cannot go stale); the device's bar is 4 x the
figure with a floor of 8 u (the series and the Newton reciprocal each add a few roundings of their own; a wrong coefficient or a missing Newton step
costs orders of magnitude).  Measured 2026-10 on the final tables:

    exp_R_small     max |R - R_ref|, so3_exp_R table, theta^2 < 0.2501 (the device's series, both edges)  host 0.81 u -> figure 0.81, device bar  8 u (the floor)
    exp_orth_small  max |R^T R - I|, the same rows                                                          host 1.45 u -> figure 1.5,  device bar  8 u (the floor)
    exp_R_large     max |R - R_ref|, the larger angles (closed form everywhere; theta up to 10)             host 12.6 u -> figure 13,   device bar 52 u
    exp_orth_large  max |R^T R - I|, the same rows                                                          host 15.5 u -> figure 16,   device bar 64 u
    solve_bwd       normwise backward error of solve_ldlt6, every system it accepts                         host 1.27 u -> figure 1.3,  device bar  8 u (the floor)
    solve_rel       |x - x_ref|_inf / |x_ref|_inf / cond(A), systems of condition <= 1e8                    host 2.15 u -> figure 2.2,  device bar  8.8 u
    try_R           max |delta[:3,:3] - R_ref(the try's own d)|, all three tables that make tries           host 0.63 u -> figure 0.64, device bar  8 u (the floor)
    try_xi          |xi - delta_ref x0| per entry, in ulps of the largest term of its sum, the same tries   host 4.97 u -> figure 5.0,  device bar 20 u
    (lambda: 0.67 ulp at most on the host; its bar is the issue's 4 ulp on both sides.  The edge check -- |R(th-) - R(th+)| against the reference's
    own difference plus the exp_R_small bar -- had 0.62 u to spare on the host.)

(the decision table's and the scripts' next tries are held to the same try_R / try_xi / solve_bwd bars).

The device on an MI355X, same tables (pytest -m gpu -s tests/test_gpu_lm_scalar.py prints them): exp_R_small 0.81 u, exp_orth_small 1.45 u, exp_R_large 12.6 u,
exp_orth_large 15.5 u, solve_bwd 1.27 u, solve_rel 2.15 u, try_R 0.63 u, try_xi 5.86 u, lambda 0.67 ulp, the edge check 0.62 u to spare: the host's
figures to three digits except try_xi (4.97 u on the host); 28 of the 64 rows between the two edges of the series differ from the host's closed form
by a bit or more, and every integer, flag and copied double of the 3744 decisions and 27 script steps equals the host's."""
import functools
import os
import subprocess
import sys

import numpy as np

import lm_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgc-slam_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "lm_device_table.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden")
LD, U = ref.LD, ref.U53

HOST_FIGURES = dict(exp_R_small=0.81, exp_orth_small=1.5, exp_R_large=13.0, exp_orth_large=16.0, solve_bwd=1.3, solve_rel=2.2, try_R=0.64, try_xi=5.0)   # units of u = 2^-53, see the module's text
LAMBDA_ULPS = 4         # pow(2 rho - 1, 3) against the cube, and one product


def bar(key, device):
    """in units of u"""
    return max(4 * HOST_FIGURES[key], 8.0) if device else HOST_FIGURES[key]


STATE = np.dtype([("x0", "f8", 16), ("lambda", "f8"), ("nu", "f8"), ("y0", "f8"), ("yi", "f8"), ("H", "f8", 36), ("b", "f8", 6), ("d", "f8", 6), ("delta", "f8", 16),
                  ("xi", "f8", 16), ("Hfin", "f8", 36), ("rot_eps", "f8"), ("trans_eps", "f8"), ("init_factor", "f8"),
                  ("phase", "i4"), ("done", "i4"), ("conv", "i4"), ("failed", "i4"), ("outer", "i4"), ("inner", "i4"), ("n_lin", "i4"), ("n_err", "i4"), ("ncorr", "i4"),
                  ("ticketA", "i4"), ("ticketB", "i4"), ("max_outer", "i4"), ("max_inner", "i4"), ("has_fit", "i4"),
                  ("fit_sum", "f8"), ("nvox", "i4"), ("def_t", "i4"), ("def_s", "i4"), ("pad", "i4"), ("gen", "i4"), ("cmd", "i4"), ("mode", "i4"), ("cur", "i4"),
                  ("src_sq", "f4"), ("pad2", "i4"), ("lazy_nq", "i4"), ("lazy_ncell", "i4")])   # rgck::LmState (csrc/rgc_kernels.h); the harness checks its size
ROW_E = np.dtype([("w", "f8", 3)])
ROW_S = np.dtype([("A", "f8", 36), ("rhs", "f8", 6)])
ROW_T = np.dtype([("H", "f8", 36), ("b", "f8", 6), ("lambda", "f8"), ("x0", "f8", 16)])
ROW_D = np.dtype([("st", STATE), ("folded", "f8", 30), ("mode", "i4"), ("cur", "i4")])
ROW_P = np.dtype([("st", STATE), ("folded", "f8", 30), ("start", "i4"), ("unused", "i4")])
OUT_E = np.dtype([("R", "f8", 9)])
OUT_S = np.dtype([("ok", "f8"), ("x", "f8", 6)])
OUT_T = np.dtype([("d", "f8", 6), ("delta", "f8", 16), ("xi", "f8", 16)])
OUT_D = np.dtype([("st", STATE), ("took_xi", "i4"), ("zero", "i4")])
MAGIC = 0x4C4D5431
# every field of the state lm_step_decide may write; the rest must come back bit for bit
WRITABLE = ("x0", "lambda", "nu", "inner", "outer", "done", "conv", "failed", "Hfin", "mode", "cur", "n_lin", "n_err", "ncorr", "y0", "yi", "H", "b", "d", "delta", "xi")
ROT_EPS, TRANS_EPS = 2.0 ** -9, 5.0e-4   # the threshold cases need 1 - rot_eps to be a double (the defaults are 2e-3 and 5e-4)


def ulps_from(x, k):
    x = np.float64(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


# ---------------------------------------------------------------- so3_exp_R
def _axes():
    rng = np.random.default_rng(20261019)
    ax = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1], [1, -1, 1]] + list(rng.standard_normal((8, 3)))
    return [np.asarray(a, np.float64) / np.linalg.norm(a) for a in ax]


def exp_cases():
    """-> list of (w, axis index, edge group or None, position in the group)"""
    lo, hi = np.sqrt(np.float64(1e-10)), np.float64(0.5)
    ths = [(0.0, None, 0), (1e-160, None, 0)] + [(ulps_from(lo, k), "lo", k) for k in range(-3, 4)] + [(t, None, 0) for t in (1e-3, 1e-2, 0.1, 0.3)]
    ths += [(ulps_from(hi, k), "hi", k) for k in range(-3, 4)] + [(t, None, 0) for t in (1.0, 3.0, np.pi, 2 * np.pi - 1e-9, 10.0)]
    return [(np.float64(th) * a, ia, grp, k) for ia, a in enumerate(_axes()) for th, grp, k in ths]


def check_exp(cases, R_out, device):
    """-> figures (units of u) and the list of violations"""
    bad, fig = [], dict(exp_R_small=0.0, exp_orth_small=0.0, exp_R_large=0.0, exp_orth_large=0.0, exp_edge=0.0)
    Rref = [ref.so3_exp_R(c[0]) for c in cases]
    for i, c in enumerate(cases):
        R = ref.ld(R_out[i]).reshape(3, 3)
        e, o = float(np.abs(R - Rref[i]).max()) / U, float(np.abs(R.T @ R - np.eye(3, dtype=LD)).max()) / U
        cl = "_small" if float(c[0] @ c[0]) < 0.2501 else "_large"    # the device's series and both edges / the closed form at large angles
        fig["exp_R" + cl], fig["exp_orth" + cl] = max(fig["exp_R" + cl], e), max(fig["exp_orth" + cl], o)
        if not e <= bar("exp_R" + cl, device):
            bad.append(("exp_R" + cl, i, c[0].tolist(), e))
        if not o <= bar("exp_orth" + cl, device):
            bad.append(("exp_orth" + cl, i, c[0].tolist(), o))
        if c[2] is not None and i + 1 < len(cases) and cases[i + 1][2] == c[2] and cases[i + 1][1] == c[1]:   # the next double along the same axis
            step = float(np.abs(ref.ld(R_out[i]) - ref.ld(R_out[i + 1])).max()) / U
            own = float(np.abs(Rref[i] - Rref[i + 1]).max()) / U
            fig["exp_edge"] = max(fig["exp_edge"], step - own)
            if not step <= own + bar("exp_R_small", device):
                bad.append(("exp_edge", i, c[0].tolist(), step, own))
    return fig, bad


# ---------------------------------------------------------------- solve_ldlt6
@functools.lru_cache(None)
def real_linearisations():
    """two real linearisations of the registration fixture (DIRECT1 and DIRECT7 at its guess): (H, b, y0, ncorr)"""
    fx = np.load(os.path.join(GOLDEN, "fx_registration.npz"))
    sym = lambda H: np.triu(H) + np.triu(H, 1).T      # (the device's sums hold the upper triangle)
    return [(sym(fx["lin_H"].astype(np.float64)), fx["lin_b"].astype(np.float64), float(fx["lin_cost"]), int(fx["lin_ncorr"])),
            (sym(fx["lin7_H"].astype(np.float64)), fx["lin7_b"].astype(np.float64), float(fx["lin7_cost"]), int(fx["lin7_ncorr"]))]


def _plane_system():
    """J^T J and J^T r of 500 point-to-plane rows [p x n, n] on one plane: rank 3"""
    rng = np.random.default_rng(7)
    n = np.array([0.0, 0.6, 0.8])
    e1, e2 = np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.8, -0.6])
    P = rng.uniform(-20, 20, (500, 1)) * e1 + rng.uniform(-20, 20, (500, 1)) * e2 + 3.0 * n
    J = np.hstack([np.cross(P, n), np.tile(n, (500, 1))])
    r = rng.normal(0, 0.02, 500)
    return J.T @ J, J.T @ r


LAMBDA_FACTORS = (1e-12, 1e-9, 1e-6, 1.0, 1e12)


@functools.lru_cache(None)
def solve_cases():
    """-> list of dict(name, H, b, lam, refused): the system is A = H + lam I, rhs = -b, as lm_try calls it.  b is scaled so that the solution's
    largest entry is at most 0.3 (a step of the registration; keeps so3_exp's argument where longdouble sin and cos need no large reduction)"""
    out = []

    def add(name, H, b, lam, refused=False):
        H, b = np.asarray(H, np.float64).reshape(6, 6), np.asarray(b, np.float64)
        if not refused:
            x = ref.solve6(H + lam * np.eye(6), -b)
            m = float(np.abs(x).max())
            if m > 0.3:
                b = b * (0.3 / m)
        out.append(dict(name=name, H=H, b=b, lam=float(lam), refused=refused))

    lins = real_linearisations()
    for i, (H, b, _, _) in enumerate(lins):                                 # (a)
        for f in LAMBDA_FACTORS:
            add(f"a{i}_{f:g}", H, b, f * np.abs(np.diag(H)).max())
    Hp, bp = _plane_system()                                                 # (b)
    for f in LAMBDA_FACTORS:
        add(f"b_{f:g}", Hp, bp, f * np.abs(np.diag(Hp)).max())
    S = np.diag([1e4] * 3 + [1e-4] * 3)                                      # (c)
    for i, (H, b, _, _) in enumerate(lins):
        for Sc in (S, np.linalg.inv(S)):
            Hs = Sc @ H @ Sc
            add(f"c{i}_{Sc[0, 0]:g}", (Hs + Hs.T) / 2, Sc @ b, 1e-9 * np.abs(np.diag(Hs)).max())
    rng = np.random.default_rng(11)                                          # (d)
    for cond in (1e2, 1e4, 1e6, 1e8, 1e10, 1e12, 1e15):
        for rep in range(3):
            Q = np.linalg.qr(rng.standard_normal((6, 6)))[0]
            A = Q @ np.diag(np.logspace(0, -np.log10(cond), 6)) @ Q.T
            add(f"d_{cond:g}_{rep}", (A + A.T) / 2, rng.standard_normal(6), 0.0)
    add("e_zero", np.zeros((6, 6)), np.zeros(6), 0.0, refused=True)          # (e)
    Hf = lins[0][0].copy(); Hf[2, 2] = 1e301                                 # (f)
    add("f_1e301", Hf, lins[0][1], 1.0, refused=True)
    L = np.eye(6) + np.tril(np.arange(36).reshape(6, 6) % 5 - 2.0, -1)       # (g) small integers: L D L^T is exact, the fourth pivot is 0.0
    add("g_pivot3", L @ np.diag([1.0, 2.0, 1.0, 0.0, 3.0, 1.0]) @ L.T, np.arange(1.0, 7.0), 0.0, refused=True)
    return out


def _A_of(c):
    A = c["H"].copy()
    A[np.diag_indices(6)] += c["lam"]          # one rounding per diagonal entry, as lm_try forms it
    return A


def check_solve(cases, ok_out, x_out, device):
    bad, fig = [], dict(solve_bwd=0.0, solve_rel=0.0)
    for i, c in enumerate(cases):
        A, rhs = _A_of(c), -c["b"]
        if bool(ok_out[i]) == c["refused"]:
            bad.append(("solve_ok", c["name"], float(ok_out[i])))
            continue
        if c["refused"]:
            continue
        be = ref.backward_error(A, x_out[i], rhs) / U
        fig["solve_bwd"] = max(fig["solve_bwd"], be)
        if not be <= bar("solve_bwd", device):
            bad.append(("solve_bwd", c["name"], be))
        cond = float(np.linalg.cond(A))
        if cond <= 1e8:
            xr = ref.solve6(A, rhs)
            rel = float(np.abs(ref.ld(x_out[i]) - xr).max() / np.abs(xr).max()) / cond / U
            fig["solve_rel"] = max(fig["solve_rel"], rel)
            if not rel <= bar("solve_rel", device):
                bad.append(("solve_rel", c["name"], rel, cond))
    return fig, bad


# ---------------------------------------------------------------- lm_try
def _poses():
    import rgc_slam_amd.synth as synth
    far = synth.se3(synth.rot_zyx(0.3, -0.2, 0.1), [1.0e4, -7.0e3, 120.0])
    return [("identity", np.eye(4)), ("turn2", synth.se3(np.asarray(ref.so3_exp_R(2.0 * _axes()[9]), np.float64), [3.0, -2.0, 0.5])), ("far", far)]


@functools.lru_cache(None)
def try_cases():
    return [dict(name=c["name"] + "/" + pn, H=c["H"], b=c["b"], lam=c["lam"], x0=x0, refused=c["refused"]) for c in solve_cases() for pn, x0 in _poses()]


def check_try(H, b, lam, x0, d, delta, xi, device, what, fig, bad, expect_nan=None):
    """one made try: d by the solve's backward error, delta and xi against the reference fed the try's OWN d (so the solve's error stays out of the
    product); NaN-ness entry for entry.  expect_nan: whether the solve must have failed (None: as the output says)"""
    d, delta, xi = np.asarray(d, np.float64), np.asarray(delta, np.float64).reshape(4, 4), np.asarray(xi, np.float64).reshape(4, 4)
    nan = bool(np.isnan(d).any())
    if expect_nan is not None and nan != expect_nan:
        bad.append(("try_failed_solve", what, nan))
        return
    if nan and not np.isnan(d).all():
        bad.append(("try_d_partly_nan", what))
    if not nan:
        A = np.asarray(H, np.float64).reshape(6, 6).copy()
        A[np.diag_indices(6)] += lam
        be = ref.backward_error(A, d, -np.asarray(b, np.float64)) / U
        fig["solve_bwd"] = max(fig.get("solve_bwd", 0.0), be)
        if not be <= bar("solve_bwd", device):
            bad.append(("try_solve_bwd", what, be))
    _, dref, xref = ref.lm_try(H, b, lam, x0, d=d)
    for name, got, want in (("delta", delta, dref), ("xi", xi, xref)):
        if not np.array_equal(np.isnan(got), np.isnan(np.asarray(want, np.float64))):
            bad.append(("try_nan_pattern", what, name))
    if not (np.array_equal(delta[:3, 3], d[3:], equal_nan=True) and np.array_equal(delta[3], [0, 0, 0, 1])):
        bad.append(("try_delta_copy", what))
    if nan:
        if not np.array_equal(xi[3], np.asarray(x0, np.float64).reshape(4, 4)[3]):
            bad.append(("try_xi_row3", what))
        return
    e = float(np.abs(ref.ld(delta[:3, :3]) - dref[:3, :3]).max()) / U
    fig["try_R"] = max(fig.get("try_R", 0.0), e)
    if not e <= bar("try_R", device):
        bad.append(("try_R", what, e))
    terms = ref.xi_terms(dref, x0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ul = np.where(terms > 0, np.abs(ref.ld(xi) - xref) / (terms * U), np.abs(ref.ld(xi) - xref))
    e = float(ul.max())
    fig["try_xi"] = max(fig.get("try_xi", 0.0), e)
    if not e <= bar("try_xi", device):
        bad.append(("try_xi", what, e))


def check_tries(cases, out, device):
    fig, bad = {}, []
    for i, c in enumerate(cases):
        check_try(c["H"], c["b"], c["lam"], c["x0"], out["d"][i], out["delta"][i], out["xi"][i], device, c["name"], fig, bad, expect_nan=c["refused"])
    return fig, bad


# ---------------------------------------------------------------- lm_step_decide
MAX_OUTER, MAX_INNER = 5, 10
RHOS = ("2", "1", "0.5", "+0", "-tiny", "-1", "+inf", "-inf", "nan")
MODES = ("LIN_first", "LIN", "BA", "B")


def junk_state():
    """a state whose every field holds something recognisable (what must not be touched is compared bit for bit)"""
    st = np.zeros((), STATE)
    for k, name in enumerate(STATE.names):
        if STATE[name].shape:
            st[name] = 1000.0 * (k + 1) + np.arange(STATE[name].shape[0])
        else:
            st[name] = 77 + k
    return st


def _delta_variants():
    """-> list of (name, delta (4x4), converged): not converged; converged; each of the twelve tested entries exactly on the threshold
    (|.| / eps == 1: not converged) and one ulp of the entry nearer its target (converged)"""
    conv = np.asarray(ref.delta_of([1e-6, -2e-6, 1.5e-6, 1e-5, -2e-5, 3e-5]), np.float64)
    out = [("far", np.asarray(ref.delta_of([0.01, 0.02, -0.01, 0.1, 0.2, 0.05]), np.float64), False), ("conv", conv, True)]
    for a in range(3):
        for e in range(4):
            target = 1.0 if a == e else 0.0
            sgn = -1.0 if (a + e) % 2 else 1.0
            v = 1.0 - ROT_EPS if a == e else sgn * (TRANS_EPS if e == 3 else ROT_EPS)
            assert abs(v - target) == (TRANS_EPS if e == 3 else ROT_EPS)                       # exact in fp64
            D = conv.copy(); D[a, e] = v
            out.append((f"at{a}{e}", D, False))
            D = conv.copy(); D[a, e] = np.nextafter(v, target)
            out.append((f"below{a}{e}", D, True))
    return out


@functools.lru_cache(None)
def decide_cases():
    """-> the ROW_D table and a list of names.  The state of every row: the registration fixture's first linearisation with b[0] = 0 and
    d = e_0, lambda = 0.75, so that d . (lambda d - b) = 0.75 exactly and rho is what y0 - yi says; the speculative linearisation in the row
    is the fixture's second."""
    (H0, b0, _, nc0), (H1, b1, y1, nc1) = real_linearisations()
    import rgc_slam_amd.synth as synth
    x0 = synth.se3(synth.rot_zyx(0.4, -0.1, 0.05), [12.0, -3.0, 0.7])
    rows, names = [], []
    for mode in MODES:
        for rho in RHOS:
            for dn, delta, _ in _delta_variants():
                for inner in (0, MAX_INNER - 1):
                    for outer in (0, MAX_OUTER - 1):
                        st = junk_state()
                        b = b0.copy(); b[0] = 0.0
                        d = np.array([1.0, 0, 0, 0, 0, 0])
                        y0, lam = 10.0, 0.75
                        if rho in ("+inf", "-inf", "nan"):
                            d = np.zeros(6)
                        if rho == "nan":
                            b = np.zeros(6)
                        yi = {"2": 8.5, "1": 9.25, "0.5": 9.625, "+0": 10.0, "-tiny": np.nextafter(10.0, 11.0), "-1": 10.75, "+inf": 9.0, "-inf": 11.0, "nan": 10.0}[rho]
                        st["x0"], st["H"], st["b"], st["d"], st["delta"] = x0.reshape(16), H0.reshape(36), b, d, delta.reshape(16)
                        st["xi"] = (delta @ x0).reshape(16)
                        st["lambda"] = -1.0 if mode == "LIN_first" else lam
                        st["nu"], st["y0"], st["yi"] = (8.0 if inner == 0 else 1024.0), y0, -5.0
                        st["Hfin"] = np.eye(6).reshape(36) * 3.0
                        st["rot_eps"], st["trans_eps"], st["init_factor"] = ROT_EPS, TRANS_EPS, 1e-9
                        st["done"] = st["conv"] = st["failed"] = 0
                        st["outer"], st["inner"], st["max_outer"], st["max_inner"] = outer, inner, MAX_OUTER, MAX_INNER
                        st["n_lin"], st["n_err"], st["ncorr"] = 3 + outer, 5 + inner, nc0
                        m = dict(LIN_first=ref.MODE_LIN, LIN=ref.MODE_LIN, BA=ref.MODE_BA, B=ref.MODE_B)[mode]
                        st["mode"], st["cur"] = m, len(rows) & 1
                        row = np.zeros((), ROW_D)
                        row["st"], row["folded"], row["mode"], row["cur"] = st, ref.fold(H1, b1, y1, nc1, yi), m, st["cur"]
                        rows.append(row)
                        names.append(f"{mode}/rho={rho}/{dn}/inner={inner}/outer={outer}")
    return np.array(rows, ROW_D), names


def state_dict(st):
    return {n: (np.array(st[n]) if STATE[n].shape else st[n].item()) for n in STATE.names}


def ulp_distance(a, b):
    """|a - b| in ulps of b (b a longdouble or a double)"""
    bd = np.float64(b)
    if not (np.isfinite(a) and np.isfinite(bd)):
        return 0.0 if (np.isnan(a) and np.isnan(bd)) or a == bd else np.inf
    return float(abs(LD(a) - LD(b)) / LD(np.spacing(abs(bd))))


def check_decision(st_in, folded, mode, cur, st_out, took_out, device, what, fig, bad):
    """one call of lm_step_decide against the reference's decision: integers, flags and copied doubles equal, lambda to LAMBDA_ULPS, the next try
    by the lm_try bars, everything else untouched"""
    e, took, nxt = ref.expect_decision(state_dict(st_in), folded, mode, cur)
    if int(took_out) != int(took):
        bad.append(("took_xi", what, int(took_out)))
    for n in STATE.names:
        got = st_out[n]
        if n == "lambda":
            u = ulp_distance(got.item(), e["lambda"])
            fig["lambda_ulps"] = max(fig.get("lambda_ulps", 0.0), u)
            if not u <= LAMBDA_ULPS:
                bad.append(("lambda", what, got.item(), float(e["lambda"]), u))
        elif n in ("d", "delta", "xi") and nxt is not None:
            continue
        else:
            want = np.asarray(e[n]).astype(STATE[n].base)
            if np.asarray(got).tobytes() != want.tobytes():
                bad.append(("field " + n + (" (must not be touched)" if n not in WRITABLE else ""), what, np.asarray(got).tolist(), want.tolist()))
    if nxt is not None:
        H, b, _, x0 = nxt
        check_try(H, b, st_out["lambda"].item(), x0, st_out["d"], st_out["delta"], st_out["xi"], device, what, fig, bad)


def check_decisions(rows, names, out, device):
    fig, bad = {}, []
    for i in range(len(rows)):
        check_decision(rows["st"][i], rows["folded"][i], int(rows["mode"][i]), int(rows["cur"][i]), out["st"][i], out["took_xi"][i], device, names[i], fig, bad)
    return fig, bad


# ---------------------------------------------------------------- scripted solves
def _lin(k, scale, y0):
    H, b, _, nc = real_linearisations()[k]
    return (H, b * scale, float(y0), nc - 7 * k)


POISON = (np.full((6, 6), 1e30), np.full(6, -1e30), 1e30, 12345)     # the speculative linearisation of a try that is NOT accepted: never adopted
# a script: the first linearisation, then the tries at the reference's level -- each try's cost yi and the linearisation that follows if it is
# accepted (None: it is rejected, or the solve ends with it).  b x 1e-6 makes a step far below the convergence thresholds.
SCRIPTS = {
    "accept_accept_converge": dict(lin0=_lin(0, 1.0, 100.0), tries=[(90.0, _lin(1, 0.5, 90.0)), (85.0, _lin(0, 1e-6, 85.0)), (84.9, None)]),
    "three_rejections_then_accept": dict(lin0=_lin(0, 1.0, 100.0), tries=[(110.0, None), (120.0, None), (105.0, None), (95.0, _lin(1, 1e-6, 95.0)), (94.5, None)]),
    "rejections_to_max_inner": dict(lin0=_lin(1, 1.0, 50.0), max_inner=4, tries=[(51.0, None), (52.0, None), (50.5, None), (60.0, None)]),
    "negative_rho_converged_delta": dict(lin0=_lin(0, 1e-6, 20.0), tries=[(21.0, None)]),
    "outer_cap_in_BA": dict(lin0=_lin(0, 1.0, 100.0), max_outer=2, tries=[(90.0, _lin(1, 0.7, 90.0)), (80.0, None)]),
    "outer_cap_in_B": dict(lin0=_lin(0, 1.0, 100.0), max_outer=2, tries=[(90.0, _lin(1, 0.7, 90.0)), (95.0, None), (85.0, None)]),
    "max_outer_1": dict(lin0=_lin(1, 1.0, 30.0), max_outer=1, tries=[(29.0, None)]),
}


def fresh_state(x0, max_outer, max_inner):
    """lm_state_open's image"""
    st = np.zeros((), STATE)
    st["x0"], st["lambda"], st["nu"], st["Hfin"] = np.asarray(x0).reshape(16), -1.0, 2.0, np.eye(6).reshape(36)
    st["rot_eps"], st["trans_eps"], st["init_factor"], st["max_outer"], st["max_inner"] = 2e-3, 5e-4, 1e-9, max_outer, max_inner
    st["mode"] = ref.MODE_LIN
    return st


@functools.lru_cache(None)
def script_cases():
    """-> the ROW_P table, and per script dict(name, first row, rows, ref = the reference loop's result, trace, modes = the launch modes)"""
    import rgc_slam_amd.synth as synth
    x0 = synth.se3(synth.rot_zyx(-0.2, 0.05, 0.3), [4.0, 9.0, -1.0])
    rows, info = [], []
    for name, s in SCRIPTS.items():
        mo, mi = s.get("max_outer", 64), s.get("max_inner", 10)
        lins = [s["lin0"]] + [l for _, l in s["tries"] if l is not None]
        yis = [y for y, _ in s["tries"]]
        res, trace = ref.solve_script(x0, lins, yis, 2e-3, 5e-4, 1e-9, mo, mi)
        assert res["n_err"] == len(yis) and res["n_lin"] == len(lins), (name, res["n_err"], res["n_lin"])   # the script is what the loop consumed
        first, modes = len(rows), [ref.MODE_LIN]
        folded, mode, nl = [ref.fold(*s["lin0"])], ref.MODE_BA, 1
        for t, (verdict, conv) in enumerate(trace):
            last = t == len(trace) - 1
            modes.append(mode)
            if mode == ref.MODE_BA:   # the speculative linearisation rides in the row, unless the try's delta is converged (the launch makes none)
                spec = (np.zeros((6, 6)), np.zeros(6), 0.0, 0) if conv else lins[nl] if verdict == ref.ACCEPT and not last else POISON
                folded.append(ref.fold(*spec, yi=yis[t]))
                if verdict == ref.ACCEPT and not last:
                    nl += 1
            else:
                folded.append(ref.fold(np.zeros((6, 6)), np.zeros(6), 0.0, 0, yi=yis[t]))
            if last:
                break
            mode = ref.NEXT_MODE[(mode, verdict)]
            if mode == ref.MODE_LIN:
                folded.append(ref.fold(*lins[nl])); nl += 1
                modes.append(ref.MODE_LIN)
                mode = ref.NEXT_MODE[(ref.MODE_LIN, "linearized")]
        assert nl == len(lins), name
        for k, f in enumerate(folded):
            row = np.zeros((), ROW_P)
            row["st"], row["folded"], row["start"] = (fresh_state(x0, mo, mi) if k == 0 else junk_state()), f, int(k == 0)
            rows.append(row)
        info.append(dict(name=name, first=first, n=len(folded), ref=res, trace=trace, modes=modes, x0=x0))
    return np.array(rows, ROW_P), info


def check_scripts(rows, info, out, device):
    """every step by check_decision (the state the step before left, the row's sums), then the finished state against the reference loop"""
    fig, bad = {}, []
    for s in info:
        for k in range(s["n"]):
            i = s["first"] + k
            st_in = rows["st"][i] if k == 0 else out["st"][i - 1]
            if int(st_in["mode"]) != s["modes"][k] or int(st_in["done"]):
                bad.append(("script_mode", s["name"], k, int(st_in["mode"]), s["modes"][k], int(st_in["done"])))
                break
            check_decision(st_in, rows["folded"][i], int(st_in["mode"]), int(st_in["cur"]), out["st"][i], out["took_xi"][i], device, f"{s['name']}[{k}]", fig, bad)
        fin, r = out["st"][s["first"] + s["n"] - 1], s["ref"]
        for n in ("outer", "conv", "failed", "n_lin", "n_err"):
            if int(fin[n]) != r[n]:
                bad.append(("script_" + n, s["name"], int(fin[n]), r[n]))
        if not int(fin["done"]):
            bad.append(("script_not_done", s["name"]))
        if not np.array_equal(fin["Hfin"].reshape(6, 6), r["Hfin"]):
            bad.append(("script_Hfin", s["name"]))
        # x0: every accepted try moves it by a step d that carries the solve's forward error, cond(H + lambda I) x the backward bar relative to a
        # step of at most 0.3 -- cond < 400 for the fixture's systems at every lambda -- and the product's few ulps of |x0| < 16
        accepted = sum(1 for v, _ in s["trace"] if v == ref.ACCEPT)
        tol = accepted * (400 * 0.3 * bar("solve_bwd", device) + 16 * (bar("try_R", device) + bar("try_xi", device))) * U
        e = float(np.abs(ref.ld(fin["x0"]).reshape(4, 4) - r["x0"]).max())
        fig["script_x0"] = max(fig.get("script_x0", 0.0), e / U)
        if not e <= tol:
            bad.append(("script_x0", s["name"], e, tol))
    return fig, bad


# ---------------------------------------------------------------- the harness
def build_harness(out, device, csrc=CSRC):
    """the stand-alone program: the host half with g++ (no GPU, no HIP runtime), both halves with hipcc for gfx950.  csrc: where rgc_lm.h and
    rgc_lm_decide.h are taken from (a scratch copy with a planted error: see tests/test_lm_reference.py)"""
    common = ["-std=c++17", "-O3", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", str(csrc), SRC, "-o", str(out)]
    if device:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950"] + common
    else:
        cmd = ["g++", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include"] + common
    subprocess.check_call(cmd)
    return str(out)


@functools.lru_cache(None)
def tables():
    E, S, T = exp_cases(), solve_cases(), try_cases()
    tE = np.zeros(len(E), ROW_E); tE["w"] = [c[0] for c in E]
    tS = np.zeros(len(S), ROW_S); tS["A"] = [_A_of(c).reshape(36) for c in S]; tS["rhs"] = [-c["b"] for c in S]
    tT = np.zeros(len(T), ROW_T); tT["H"] = [c["H"].reshape(36) for c in T]; tT["b"] = [c["b"] for c in T]; tT["lambda"] = [c["lam"] for c in T]
    tT["x0"] = [c["x0"].reshape(16) for c in T]
    return tE, tS, tT, decide_cases()[0], script_cases()[0]


def run_harness(exe, workdir, host_only):
    """one child process, a time limit -> dict(host=..., device=... or None) of the five result tables"""
    tabs = tables()
    assert STATE.itemsize == 1224 and ROW_D.itemsize == 1472 and OUT_D.itemsize == 1232
    fin, fout = os.path.join(str(workdir), "lm_tables.bin"), os.path.join(str(workdir), "lm_results.bin")
    with open(fin, "wb") as f:
        f.write(np.array([MAGIC, STATE.itemsize] + [len(t) for t in tabs] + [0], np.int32).tobytes())
        for t in tabs:
            f.write(t.tobytes())
    r = subprocess.run([exe] + (["--host-only"] if host_only else []) + [fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    hdr = np.frombuffer(raw, np.int32, 8)
    assert hdr[0] == MAGIC and hdr[7] == (0 if host_only else 1)
    off, res = 32, {}
    for half in ("host",) + (() if host_only else ("device",)):
        got = []
        for t, dt in zip(tabs, (OUT_E, OUT_S, OUT_T, OUT_D, OUT_D)):
            got.append(np.frombuffer(raw, dt, len(t), off)); off += len(t) * dt.itemsize
        res[half] = got
    assert off == len(raw)
    return res


def check_all(got, device):
    """-> {table: (figures, violations)} of one half's five result tables"""
    tE, tS, tT, tD, tP = tables()
    return dict(exp=check_exp(exp_cases(), got[0]["R"], device), solve=check_solve(solve_cases(), got[1]["ok"], got[1]["x"], device),
                tries=check_tries(try_cases(), got[2], device), decide=check_decisions(tD, decide_cases()[1], got[3], device),
                scripts=check_scripts(tP, script_cases()[1], got[4], device))


if __name__ == "__main__":   # python tests/lm_cases.py [--device] [--csrc <directory>] [--device-bars: hold the host half to the device's bars]
    import tempfile
    sys.path.insert(0, ROOT)
    csrc = sys.argv[sys.argv.index("--csrc") + 1] if "--csrc" in sys.argv else CSRC
    with tempfile.TemporaryDirectory() as td:
        res = run_harness(build_harness(os.path.join(td, "lm_device_table"), "--device" in sys.argv, csrc), td, host_only="--device" not in sys.argv)
    for half, got in res.items():
        for table, (fig, bad) in check_all(got, half == "device" or "--device-bars" in sys.argv).items():
            print(half, table, {k: round(v, 3) for k, v in fig.items()}, f"{len(bad)} violations", *bad[:5], sep="\n  " if bad else " ")
