"""numpy longdouble reference of the scalar step of LsqRegistration's Levenberg-Marquardt (so3/so3.hpp:58-77, lsq_registration_impl.hpp:82-91,
125-172): so3_exp as a rotation matrix, a pivoted 6x6 solve, one LM try, the convergence test, step_lm's decision after one try, the loop over a
scripted solve, and -- as data -- which launch mode of the device route follows which decision.  Written from the reference's text; it takes nothing
from oracle/ and nothing from csrc/rgc_lm.h.  Everything is np.longdouble (x87 extended here: 64-bit significand) unless a name says otherwise."""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53


def ld(a):
    return np.asarray(a, dtype=LD)


def so3_exp_R(w):
    """so3_exp (so3.hpp:58-77) followed by Quaterniond::toRotationMatrix, the closed form at every angle (the reference's own series below
    theta^2 = 1e-10 truncates at theta^6 / 46080 < 1e-34)"""
    w = ld(w)
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if th2 == 0:
        imag, real = LD(0.5), LD(1)
    else:
        th = np.sqrt(th2)
        half = th / 2
        imag, real = np.sin(half) / th, np.cos(half)
    qw, qx, qy, qz = real, imag * w[0], imag * w[1], imag * w[2]
    R = np.empty((3, 3), dtype=LD)
    R[0, 0] = 1 - 2 * (qy * qy + qz * qz); R[0, 1] = 2 * (qx * qy - qz * qw); R[0, 2] = 2 * (qx * qz + qy * qw)
    R[1, 0] = 2 * (qx * qy + qz * qw); R[1, 1] = 1 - 2 * (qx * qx + qz * qz); R[1, 2] = 2 * (qy * qz - qx * qw)
    R[2, 0] = 2 * (qx * qz - qy * qw); R[2, 1] = 2 * (qy * qz + qx * qw); R[2, 2] = 1 - 2 * (qx * qx + qy * qy)
    return R


def solve6(A, rhs):
    """A x = rhs by Gaussian elimination with partial pivoting; None where a pivot column is all zero or not finite"""
    A, x = ld(A).copy().reshape(6, 6), ld(rhs).copy()
    for k in range(6):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if not np.isfinite(A[p, k]) or A[p, k] == 0:
            return None
        if p != k:
            A[[k, p]] = A[[p, k]]
            x[[k, p]] = x[[p, k]]
        for i in range(k + 1, 6):
            m = A[i, k] / A[k, k]
            A[i, k:] -= m * A[k, k:]
            x[i] -= m * x[k]
    for k in range(5, -1, -1):
        x[k] = (x[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def backward_error(A, x, rhs):
    """normwise: |A x - rhs|_inf / (|A|_inf |x|_inf + |rhs|_inf)"""
    A, x, rhs = ld(A).reshape(6, 6), ld(x), ld(rhs)
    return float(np.abs(A @ x - rhs).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(rhs).max()))


def delta_of(d):
    d = ld(d)
    D = np.zeros((4, 4), dtype=LD)
    D[:3, :3] = so3_exp_R(d[:3])
    D[:3, 3] = d[3:]
    D[3, 3] = 1
    return D


def lm_try(H, b, lam, x0, d=None):
    """:136-143.  d given: the solve is taken as that (a NaN d is a failed solve) -> d, delta, xi"""
    if d is None:
        d = solve6(ld(H).reshape(6, 6) + LD(lam) * np.eye(6, dtype=LD), -ld(b))
        if d is None:
            d = np.full(6, np.nan, dtype=LD)
    delta = delta_of(d)
    with np.errstate(invalid="ignore"):
        xi = delta @ ld(x0).reshape(4, 4)
    return ld(d), delta, xi


def xi_terms(delta, x0):
    """the largest |term| of each entry's sum in delta x0 (what an ulp of that entry is measured in)"""
    d, x = np.abs(ld(delta)).reshape(4, 4), np.abs(ld(x0)).reshape(4, 4)
    return (d[:, :, None] * x[None, :, :]).max(axis=1)


def is_converged(delta, rot_eps, trans_eps):
    """:82-91, with |.| / eps for 1 / eps * |.| (the same number before rounding)"""
    delta = ld(delta).reshape(4, 4)
    m = max((np.abs(delta[:3, :3] - np.eye(3, dtype=LD)) / LD(rot_eps)).max(), (np.abs(delta[:3, 3]) / LD(trans_eps)).max())
    return bool(m < 1)


ACCEPT, REJECT, END_OUTER, NOT_CONVERGED = "accept", "reject", "end of outer iteration", "lm not converged"


def step_lm_try(x0, lam, nu, inner, H, b, y0, d, delta, xi, yi, rot_eps, trans_eps, max_inner):
    """One pass of step_lm's loop body from :145 on, for the try (d, delta, xi) whose cost is yi, the loop counter at `inner`.
    -> verdict, x0, lambda, nu, final_hessian (None: not written)"""
    d, b = ld(d), ld(b)
    lam = LD(lam)
    with np.errstate(all="ignore"):
        rho = (LD(y0) - LD(yi)) / (d @ (lam * d - b))   # :145
        if rho < 0:                                      # :155
            if is_converged(delta, rot_eps, trans_eps):
                return END_OUTER, x0, lam, nu, None      # return true, x0 as it was
            lam, nu = LD(nu) * lam, 2 * nu               # :160-161
            if inner + 1 >= max_inner:                   # the for loop runs out: return false
                return NOT_CONVERGED, x0, lam, nu, None
            return REJECT, x0, lam, nu, None
        c = 1 - np.power(2 * rho - 1, 3)                 # :166, std::max(a, b) = a < b ? b : a
        third = LD(1) / 3
        lam = lam * (c if third < c else third)
    return ACCEPT, xi, lam, nu, H


MODE_LIN, MODE_BA, MODE_B = 0, 1, 2
# the launch modes of the device route (k_lm_step's comment): what the launch after a decision does.  None: no launch follows from the verdict alone
NEXT_MODE = {(MODE_LIN, "linearized"): MODE_BA,
             (MODE_BA, ACCEPT): MODE_BA, (MODE_BA, REJECT): MODE_B,
             (MODE_B, ACCEPT): MODE_LIN, (MODE_B, REJECT): MODE_B}


def unfold(folded):
    """folded[30] -> H (6x6), b, y0, ncorr, yi: 21 upper-triangular H, 6 b, y0, ncorr, yi"""
    f = np.asarray(folded, dtype=np.float64)
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = f[:21]
    H = H + np.triu(H, 1).T
    return H, f[21:27].copy(), f[27], int(f[28]), f[29]


def fold(H, b, y0, ncorr, yi=0.0):
    return np.concatenate([np.asarray(H, np.float64).reshape(6, 6)[np.triu_indices(6)], np.asarray(b, np.float64), [y0, float(ncorr), yi]])


def expect_decision(st, folded, mode, cur):
    """What a launch's decision must leave of the state `st` (a dict of the LmState's fields, doubles as float64) given that launch's folded
    sums, in the terms of the reference's loop.  -> the state after (only fields that change are replaced; lambda is a longdouble), took_xi,
    and the next try's (H, b, lambda, x0) or None where none is made."""
    e = dict(st)
    Hf, bf, y0f, ncf, yi = unfold(folded)

    def adopt():
        e.update(H=Hf.reshape(36).copy(), b=bf.copy(), y0=y0f, ncorr=ncf, n_lin=e["n_lin"] + 1)

    if mode == MODE_LIN:                                  # :128-132, then the first try
        adopt()
        if st["lambda"] < 0:
            e["lambda"] = LD(st["init_factor"]) * LD(np.abs(np.diag(Hf)).max())
        e["mode"] = NEXT_MODE[(MODE_LIN, "linearized")]
        return e, False, (e["H"], e["b"], e["lambda"], e["x0"])
    e["yi"] = yi
    e["n_err"] = st["n_err"] + 1
    verdict, x0, lam, nu, Hfin = step_lm_try(st["x0"], st["lambda"], st["nu"], st["inner"], st["H"], st["b"], st["y0"], st["d"], st["delta"], st["xi"], yi,
                                             st["rot_eps"], st["trans_eps"], st["max_inner"])
    e["lambda"] = lam
    if verdict == NOT_CONVERGED:                          # :69-72
        e.update(nu=nu, inner=st["inner"] + 1, failed=1, done=1)
        return e, False, None
    if verdict == REJECT:
        e.update(nu=nu, inner=st["inner"] + 1, mode=NEXT_MODE[(mode, REJECT)])
        return e, False, (st["H"], st["b"], lam, st["x0"])
    # step_lm returned true: the outer loop's :74 and :65
    took = verdict == ACCEPT
    if took:
        e.update(x0=np.asarray(x0, np.float64).copy(), Hfin=np.asarray(Hfin, np.float64).copy())
    conv = is_converged(st["delta"], st["rot_eps"], st["trans_eps"])
    e.update(conv=int(conv), outer=st["outer"] + 1, nu=2.0, inner=0)
    if conv or e["outer"] >= st["max_outer"]:
        e["done"] = 1
        return e, took, None
    assert took                                           # (END_OUTER is converged by definition)
    e["mode"] = NEXT_MODE[(mode, ACCEPT)]
    if mode == MODE_BA:                                   # the speculative linearisation was taken at xi, the new x0
        adopt()
        e["cur"] = cur ^ 1
        return e, True, (e["H"], e["b"], lam, e["x0"])
    return e, True, None                                  # the next launch linearises


def solve_script(x0, lins, yis, rot_eps, trans_eps, init_factor, max_outer, max_inner):
    """computeTransformation (:53-79) over a script: lins = the linearisations (H, b, y0, ncorr) in the order the loop asks for them, yis = the costs
    of the tries in the order it makes them.  -> dict(x0, outer, conv, failed, Hfin, n_lin, n_err, lambda) and the trace [(verdict, delta converged)]"""
    x0 = ld(x0).reshape(4, 4)
    lam, conv, failed = LD(-1), False, False
    Hfin = np.eye(6)
    n_lin = n_err = outer = 0
    trace = []
    for it in range(max_outer):
        if conv:
            break
        H, b, y0, _ = lins[n_lin]; n_lin += 1             # :128
        if lam < 0:
            lam = LD(init_factor) * LD(np.abs(np.diag(np.asarray(H).reshape(6, 6))).max())
        nu, ok = 2.0, False
        for k in range(max_inner):
            d, delta, xi = lm_try(H, b, lam, x0)
            yi = yis[n_err]; n_err += 1
            verdict, x0n, lam, nu, Hf = step_lm_try(x0, lam, nu, k, H, b, y0, d, delta, xi, yi, rot_eps, trans_eps, max_inner)
            trace.append((verdict, is_converged(delta, rot_eps, trans_eps)))
            if verdict in (REJECT, NOT_CONVERGED):
                continue
            if verdict == ACCEPT:
                x0, Hfin = x0n, np.asarray(Hf, np.float64).reshape(6, 6)
            ok = True
            break
        outer = it + 1
        if not ok:
            failed = True
            outer = it                                    # the device counts finished outer iterations
            break
        conv = is_converged(delta, rot_eps, trans_eps)
    return dict(x0=x0, outer=outer, conv=int(conv), failed=int(failed), Hfin=Hfin, n_lin=n_lin, n_err=n_err, lam=lam), trace
