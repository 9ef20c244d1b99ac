"""An independent numpy reference of the 4-DoF pose graph (rgc_pgo_*), written from the mapping node's PoseGraphOptimize4DoF
(src/RGC_mapping.cpp:2303-2466), its loop edge (:2086-2107) and FourDOFError / AngleLocalParameterization / NormalizeAngle /
YawPitchRollToRotationMatrix (src/lidarFactor.hpp:490-595) -- not from the kernels: dense matrices, one edge after the other, np.longdouble
unless a dtype is asked for.  The LM loop is tests/mapreg_reference.py's lm_solve generalised to this problem."""
import numpy as np

LD = np.longdouble
RAD2DEG = 180.0 / np.pi      # :197
DEG2RAD = np.pi / 180.0
MAX_LOOPS = 128
OPTIMIZED, NO_LOOP = 0, 1


def normalize_angle(a):
    """NormalizeAngle, src/lidarFactor.hpp:490-499: one wrap at +-180"""
    if a > 180.0:
        return a - 360.0
    if a < -180.0:
        return a + 360.0
    return a


def ypr_matrix(yaw, pitch, roll, dt=LD):
    """YawPitchRollToRotationMatrix (:517-533) = Utility::ypr2R (utility.h:123-147), degrees in; also dR/dyaw per radian"""
    pi = dt(np.pi)
    y, p, r = dt(yaw) / dt(180.0) * pi, dt(pitch) / dt(180.0) * pi, dt(roll) / dt(180.0) * pi
    cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    R = np.array([[cy * cp, -sy * cr + cy * sp * sr, sy * sr + cy * sp * cr],
                  [sy * cp, cy * cr + sy * sp * sr, -cy * sr + sy * sp * cr],
                  [-sp, cp * sr, cp * cr]], dtype=dt)
    dR = np.array([[-sy * cp, -cy * cr - sy * sp * sr, cy * sr - sy * sp * cr],
                   [cy * cp, -sy * cr + cy * sp * sr, sy * sr + cy * sp * cr],
                   [0, 0, 0]], dtype=dt)
    return R, dR


def state_of(poses):
    """(:2352-2358) poses (N, 6) float32 {x, y, z, roll, pitch, yaw} -> x (N, 4) float64 {yaw_deg, t}, pitch_deg (N), roll_deg (N)"""
    p = np.asarray(poses, np.float32).reshape(-1, 6)
    x = np.empty((p.shape[0], 4), np.float64)
    x[:, 0] = p[:, 5].astype(np.float64) * RAD2DEG
    x[:, 1:4] = p[:, 0:3].astype(np.float64)
    return x, p[:, 4].astype(np.float64) * RAD2DEG, p[:, 3].astype(np.float64) * RAD2DEG


def poses_of(x, poses):
    """write-back (:2450-2455): x, y, z = (float) t, yaw = (float)(yaw_deg * deg2rad); pitch and roll as stored"""
    out = np.array(poses, np.float32).reshape(-1, 6).copy()
    x = np.asarray(x, np.float64).reshape(-1, 4)
    out[:, 0:3] = x[:, 1:4].astype(np.float32)
    out[:, 5] = (x[:, 0] * DEG2RAD).astype(np.float32)
    return out


def build_graph(ids, poses, loops):
    """ids (N) in the caller's order, poses (N, 6) float32 of those ids, loops: dicts(key_curr, key_loop, t (3), yaw, pitch, roll) [degrees].
    Returns dict(status, ij (E, 2), meas (E, 6) float64, fixed (position or -1), fixed_id, used (indices), n_ignored) or None where the call is
    refused (a repeated id, a loop onto itself, more than MAX_LOOPS used loops, non-finite loop data)."""
    ids = [int(i) for i in ids]
    N = len(ids)
    if N < 1 or len(set(ids)) != N:
        return None
    pos = {k: i for i, k in enumerate(ids)}
    x, pitch, roll = state_of(poses)
    ij, meas = [], []
    for i in range(1, N):                                            # :2367-2373
        R, _ = ypr_matrix(x[i - 1, 0], pitch[i - 1], roll[i - 1], LD)   # q_array[keyFrom] = ypr2R(...)
        m = R.T @ (x[i, 1:4].astype(LD) - x[i - 1, 1:4].astype(LD))
        ij.append((i - 1, i))
        meas.append([float(m[0]), float(m[1]), float(m[2]), x[i, 0] - x[i - 1, 0], pitch[i - 1], roll[i - 1]])
    used, ignored, oldest = [], 0, None
    for k, L in enumerate(loops):
        vals = list(L["t"]) + [L["yaw"], L["pitch"], L["roll"]]
        if not np.all(np.isfinite(vals)) or L["key_curr"] == L["key_loop"]:
            return None
        if L["key_curr"] not in pos or L["key_loop"] not in pos or pos[L["key_curr"]] == 0:   # :2364 precedes :2376
            ignored += 1
            continue
        used.append(k)
        if oldest is None or L["key_loop"] < oldest:
            oldest = L["key_loop"]
    if len(used) > MAX_LOOPS:
        return None
    for k in used:
        L = loops[k]
        ij.append((pos[L["key_loop"]], pos[L["key_curr"]]))
        meas.append([float(L["t"][0]), float(L["t"][1]), float(L["t"][2]), float(L["yaw"]), float(L["pitch"]), float(L["roll"])])
    return dict(status=OPTIMIZED if used else NO_LOOP, N=N, ij=np.array(ij, np.int32).reshape(-1, 2), meas=np.array(meas, np.float64).reshape(-1, 6),
                fixed=pos[oldest] if used else -1, fixed_id=oldest if used else -1, used=used, n_ignored=ignored)


def edge_terms(ij, meas, x, fixed, dt=LD):
    """residuals (E, 4) and the analytic Jacobians Ji, Jj (E, 4, 4; columns yaw, tx, ty, tz) of every edge at x (N, 4)"""
    E = len(ij)
    r, Ji, Jj = np.zeros((E, 4), dt), np.zeros((E, 4, 4), dt), np.zeros((E, 4, 4), dt)
    x = np.asarray(x).astype(dt)
    m = np.asarray(meas).astype(dt)
    for e in range(E):
        i, j = int(ij[e][0]), int(ij[e][1])
        R, dR = ypr_matrix(x[i, 0], m[e, 4], m[e, 5], dt)
        d = x[j, 1:4] - x[i, 1:4]
        r[e, 0:3] = R.T @ d - m[e, 0:3]
        r[e, 3] = normalize_angle(x[j, 0] - x[i, 0] - m[e, 3])
        Ji[e, 0:3, 0] = (dt(np.pi) / dt(180.0)) * (dR.T @ d)
        Ji[e, 0:3, 1:4] = -R.T
        Ji[e, 3, 0] = -1
        Jj[e, 0:3, 1:4] = R.T
        Jj[e, 3, 0] = 1
        if i == fixed:
            Ji[e] = 0
        if j == fixed:
            Jj[e] = 0
    return r, Ji, Jj


def evaluate(graph, x, dt=LD):
    """dense H (4N, 4N), g (4N), cost, the sums of the magnitudes of their terms (absH, absg), the residuals and the per-edge blocks;
    one edge after the other in dtype dt (LD: the reference; float64: the plain sequential evaluation the tolerance is measured with)"""
    N, ij = graph["N"], graph["ij"]
    r, Ji, Jj = edge_terms(ij, graph["meas"], x, graph["fixed"], dt)
    H, aH = np.zeros((4 * N, 4 * N), dt), np.zeros((4 * N, 4 * N), dt)
    g, ag = np.zeros(4 * N, dt), np.zeros(4 * N, dt)
    cost = dt(0)
    off = np.zeros((len(ij), 4, 4), dt)
    for e in range(len(ij)):
        i, j = int(ij[e][0]), int(ij[e][1])
        si, sj = slice(4 * i, 4 * i + 4), slice(4 * j, 4 * j + 4)
        for k in range(4):                                    # the residual's rows one after the other
            a, b = Ji[e, k], Jj[e, k]
            H[si, si] += np.outer(a, a); aH[si, si] += np.abs(np.outer(a, a))
            H[sj, sj] += np.outer(b, b); aH[sj, sj] += np.abs(np.outer(b, b))
            H[si, sj] += np.outer(a, b); aH[si, sj] += np.abs(np.outer(a, b))
            H[sj, si] += np.outer(b, a); aH[sj, si] += np.abs(np.outer(b, a))
            off[e] += np.outer(a, b)
            g[si] += a * r[e, k]; ag[si] += np.abs(a * r[e, k])
            g[sj] += b * r[e, k]; ag[sj] += np.abs(b * r[e, k])
        cost += (r[e] * r[e]).sum() / 2
    return dict(H=H, g=g, cost=cost, absH=aH, absg=ag, r=r, off=off)


def blocks_of(graph, ev):
    """the read-out's layout from a dense evaluation: H_diag (N, 4, 4), H_chain (N - 1, 4, 4), H_loop (L, 4, 4) -- an off-diagonal block is its
    edge's own term -- with the matching magnitude sums"""
    N, ij = graph["N"], graph["ij"]
    H, aH = ev["H"], ev["absH"]
    Hd = np.stack([H[4 * n:4 * n + 4, 4 * n:4 * n + 4] for n in range(N)])
    aHd = np.stack([aH[4 * n:4 * n + 4, 4 * n:4 * n + 4] for n in range(N)])
    off = ev["off"]
    return dict(H_diag=Hd, abs_diag=aHd, H_chain=off[:N - 1], H_loop=off[N - 1:], n_chain=N - 1)


def deviation(got, want, scale):
    """mapreg_reference.deviation's unit: the largest |difference| / sum |terms of that entry|, and whether every entry whose terms are all
    exactly zero is exactly zero"""
    got, want, scale = np.asarray(got).astype(LD), np.asarray(want).astype(LD), np.asarray(scale).astype(LD)
    nz = scale > 0
    dev = float(np.max(np.abs(got - want)[nz] / scale[nz])) if nz.any() else 0.0
    return dev, bool(np.all(got[~nz] == 0))


def term_deviation(graph, x, got, ref=None):
    """the deviation of a read-out `got` (dict g (N, 4), cost, H_diag, H_chain, H_loop) from the longdouble reference at x"""
    ev = ref if ref is not None else evaluate(graph, x, LD)
    bl = blocks_of(graph, ev)
    dev, zeros = 0.0, True
    pairs = [(np.asarray(got["g"]).reshape(-1), ev["g"], ev["absg"]), (got["H_diag"], bl["H_diag"], bl["abs_diag"])]
    off_got = np.concatenate([np.asarray(got["H_chain"]).reshape(-1, 4, 4), np.asarray(got["H_loop"]).reshape(-1, 4, 4)]) if len(graph["ij"]) else np.zeros((0, 4, 4))
    off_want = ev["off"]
    # an off-diagonal block is ONE edge's term: four products per entry
    r, Ji, Jj = edge_terms(graph["ij"], graph["meas"], x, graph["fixed"], LD)
    off_abs = np.einsum("eka,ekb->eab", np.abs(Ji), np.abs(Jj))
    pairs.append((off_got, off_want, off_abs))
    for a, b, s in pairs:
        d, z = deviation(a, b, s)
        dev, zeros = max(dev, d), zeros and z
    if ev["cost"] > 0:
        dev = max(dev, float(abs(LD(got["cost"]) - ev["cost"]) / ev["cost"]))
    else:
        zeros = zeros and got["cost"] == 0
    return dev, zeros


def fp64_readout(graph, x):
    """the plain sequential fp64 numpy evaluation of the same formulas, in the read-out's layout"""
    ev = evaluate(graph, x, np.float64)
    bl = blocks_of(graph, ev)
    return dict(g=ev["g"].reshape(-1, 4), cost=float(ev["cost"]), H_diag=bl["H_diag"], H_chain=bl["H_chain"], H_loop=bl["H_loop"])


def free_index(graph):
    N, f = graph["N"], graph["fixed"]
    return np.array([4 * n + k for n in range(N) if n != f for k in range(4)], dtype=np.int64)


def damped_system(H, g, radius, idx):
    """(H + clamp(diag H, 1e-6, 1e32) / radius) and -g over the free parameters"""
    A = H[np.ix_(idx, idx)].copy()
    dg = np.clip(np.diag(A), 1e-6, 1e32)
    A[np.diag_indices_from(A)] += dg / type(dg[0])(radius)
    return A, -g[idx]


def cholesky_solve_ld(A, b):
    """longdouble dense Cholesky, column by column; None where the matrix is not positive definite"""
    A, b = A.astype(LD), b.astype(LD)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            return None
        L[j:, j] = v / np.sqrt(v[0])
    y = np.zeros(n, LD)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def step_ld(graph, ev, radius):
    """the LM step d (N, 4) of the damped system by the longdouble Cholesky (zero on the constant node)"""
    idx = free_index(graph)
    A, b = damped_system(ev["H"], ev["g"], radius, idx)
    s = cholesky_solve_ld(A, b)
    d = np.zeros(4 * graph["N"], LD)
    d[idx] = s
    return d.reshape(-1, 4)


def step_fp64(graph, ev, radius):
    """the same system rounded to fp64 and solved by np.linalg.solve (LAPACK's pivoted LU: another elimination order)"""
    idx = free_index(graph)
    A, b = damped_system(ev["H"].astype(np.float64), ev["g"].astype(np.float64), radius, idx)
    d = np.zeros(4 * graph["N"])
    d[idx] = np.linalg.solve(A, b)
    return d.reshape(-1, 4)


def step_deviation(d, d_ref):
    d, d_ref = np.asarray(d).astype(LD), np.asarray(d_ref).astype(LD)
    return float(np.max(np.abs(d - d_ref)) / np.max(np.abs(d_ref)))


def plus(x, d, fixed):
    """AngleLocalParameterization (:501-515) on the yaw, additive on t; the constant node stays"""
    xn = np.array(x, np.float64).reshape(-1, 4).copy()
    d = np.asarray(d, np.float64).reshape(-1, 4)
    for n in range(xn.shape[0]):
        if n == fixed:
            continue
        xn[n, 0] = normalize_angle(xn[n, 0] + d[n, 0])
        xn[n, 1:4] += d[n, 1:4]
    return xn


def lm_solve(graph, x0, max_iterations=10, initial_radius=1e4):
    """Ceres' trust-region LM as the mapping node configures it (:2423-2427: max_num_iterations = 10, defaults otherwise), the restatement of
    mapreg_reference.lm_solve in dimension 4 (N - 1): gradient tolerance 1e-10 (max norm), damping clamp(diag H, 1e-6, 1e32) / radius, a step
    is accepted above a relative decrease of 1e-3, the radius grows by 1 / max(1/3, 1 - (2 rho - 1)^3) (<= 1e16) or shrinks by 2, 4, 8 ...;
    function tolerance 1e-6, parameter tolerance 1e-8 over the free parameters, minimum radius 1e-32.  H, g, cost: evaluate() (longdouble)
    rounded to double; the loop runs in double.  Returns x, dict(iterations, successful, stop, steps=[dict(rho, accepted, radius, dcost,
    step_norm, x_norm)], initial_cost, final_cost)."""
    idx = free_index(graph)

    def ev(xv):
        e = evaluate(graph, xv, LD)
        return e["H"].astype(np.float64), e["g"].astype(np.float64), float(e["cost"])
    x = np.array(x0, np.float64).reshape(-1, 4)
    radius, dec = float(initial_radius), 2.0
    H, g, cost = ev(x)
    out = dict(initial_cost=cost, successful=0, steps=[])
    it, stop = 0, "cap"
    while it < max_iterations:
        if np.abs(g).max() <= 1e-10:
            stop = "gradient"
            break
        A, b = damped_system(H, g, radius, idx)
        try:
            L = np.linalg.cholesky(A)
            s = np.linalg.solve(L.T, np.linalg.solve(L, b))
            d = np.zeros(H.shape[0])
            d[idx] = s
            model = float(-d @ (g + 0.5 * H @ d))
        except np.linalg.LinAlgError:
            model, d = -1.0, np.zeros(H.shape[0])
        rho = -1.0
        if model > 0:
            xn = plus(x, d, graph["fixed"])
            Hn, gn, newc = ev(xn)
            rho = (cost - newc) / model
        it += 1
        stop = "cap"
        if rho > 1e-3:
            old = cost
            x, H, g, cost = xn, Hn, gn, newc
            radius = min(radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 1e16)
            dec = 2.0
            out["successful"] += 1
            sn, xnorm = float(np.linalg.norm(d)), float(np.linalg.norm(x.reshape(-1)[idx]))
            out["steps"].append(dict(rho=rho, accepted=True, radius=radius, dcost=abs(old - cost) / old, step_norm=sn, x_norm=xnorm))
            if abs(old - cost) <= 1e-6 * old:
                stop = "function"
                break
            if sn <= 1e-8 * (xnorm + 1e-8):
                stop = "parameter"
                break
        else:
            radius /= dec
            dec *= 2.0
            out["steps"].append(dict(rho=rho, accepted=False, radius=radius, dcost=None, step_norm=None, x_norm=None))
            if radius < 1e-32:
                stop = "radius"
                break
    out.update(final_cost=cost, iterations=it, stop=stop)
    return x, out


def pcl_transformation(pose, dt=np.float32):
    """pclPointToAffine3f (:2614-2617) = pcl::getTransformation(x, y, z, roll, pitch, yaw), in float"""
    x, y, z, roll, pitch, yaw = [dt(v) for v in np.asarray(pose, np.float32)]
    A, B, C, D, E, F = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    DE, DF = D * E, D * F
    return np.array([[A * C, A * DF - B * E, B * F + A * DE, x], [B * C, A * E + B * DF, B * DE - A * F, y], [-D, C * F, C * E, z], [0, 0, 0, 1]], dtype=dt)


def make_loop(latest_pose, loop_pose, T_drift, key_curr, key_loop, dt=np.float32):
    """the loop edge of :2086-2107: T_loop_correct = T_w_loop^-1 T_drift T_w_latest (Affine3f: dt = float32; float64 gives the exact-arithmetic
    yardstick), its translation, R2ypr of its rotation (utility.h:105-121, fp64), the loop pose's pitch and roll in degrees"""
    Tl, Tw = pcl_transformation(latest_pose, dt), pcl_transformation(loop_pose, dt)
    Td = np.asarray(T_drift, np.float32).reshape(4, 4).astype(dt)
    Ti = np.eye(4, dtype=dt)
    Ti[:3, :3] = Tw[:3, :3].T
    Ti[:3, 3] = -(Tw[:3, :3].T @ Tw[:3, 3])
    T = (Ti @ (Td @ Tl)).astype(np.float64)
    yaw = np.arctan2(T[1, 0], T[0, 0])
    lp = np.asarray(loop_pose, np.float32)
    return dict(key_curr=int(key_curr), key_loop=int(key_loop), t=T[:3, 3].copy(), yaw=yaw / np.pi * 180.0, pitch=float(lp[4]) * RAD2DEG, roll=float(lp[3]) * RAD2DEG)
