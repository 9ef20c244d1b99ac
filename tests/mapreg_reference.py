"""An independent reference of the mapping node's feature-registration SOLVE (f1, everything behind the association): numpy, np.longdouble,
analytic Jacobians, written from the cost functors of src/lidarFactor.hpp -- LidarEdgeFactor (:9-51), LidarPlaneNormFactor (:91-121),
RelativeRFactor (:174-226), Ground_DeltaFactor_goable (:352-403), Quaternion2EulerAngle / PitchRollFactor (:405-468) -- and from Ceres'
published LM.  It is neither the kernel's code nor the C oracle's: TEST INFRASTRUCTURE ONLY.

Derivation.  A pose is (q, t), q = x,y,z,w; v -> q v is Eigen's quaternion * vector, v + w u + q_xyz x u with u = 2 q_xyz x v.
EigenQuaternionParameterization::Plus is q' = dq (x) q with dq = (sin|d| / |d| d, cos|d|): a rotation by the angle 2|d| about d applied
on the LEFT.  To first order dq = (d, 1) and (dq (x) q) v = q v + 2 d x (q v), so with Rp = q p

    d(Rp)/dd = -2 [Rp]x        (the library's scaling: d is HALF the rotation vector),        d(Rp + t)/dt = I.

Every Jacobian below is built column by column from that differential: for the tangent direction c the world point moves by
dlp_c = 2 e_c x Rp (c < 3) or e_{c-3} (c >= 3), and the residual's own differential is applied to dlp_c.
  edge    r = s (lp - a) x (lp - b), s = var / |a - b|:    d((lp - a) x (lp - b)) = dlp x ((lp - b) - (lp - a)) = dlp x (a - b)
  plane   r = var (n . lp + d):                            dr = var n . dlp
  ground  gn = ql* (q cn) (ql the fixed last pose), t_lc = ql* (t - tl), r0 = (d_last - d_cur - (qh t_lc)_z) / (p_var / 1000),
          r1,2 = |v1,2 . gn| / (10 p_var):  dr0/dd = 0, dr0/dt_c = -(qh (ql* e_c))_z / (p_var / 1000);
          dr1/dd_c = sign(v1 . gn) v1 . (ql* (2 e_c x (q cn))) / (10 p_var), dr1/dt = 0  (autodiff's abs() is sign(); the kink is v . gn = 0)
  IMU     e = A (x) q_cur with A = dq_imu* (x) q_last*, r0..2 = 2 e_xyz / imu_cov.  q_cur' = (d,1) (x) q_cur gives de_c = A (x) (e_c,0) (x) q_cur;
          q_last' = (d,1) (x) q_last gives q_last'* = q_last* (x) (-d,1), so de_c = -A (x) (e_c,0) (x) q_cur: the two 3 x 3 blocks are
          opposite.  pitch = asin(sinp), sinp = 2 (w y - x z), clamped to +-pi/2 where |sinp| >= 1 (a constant there: derivative 0);
          roll = atan2(sr, cr), sr = 2 (w x + y z), cr = 1 - 2 (x^2 + y^2); with dq_c = (e_c,0) (x) q:
          dpitch = dsinp / sqrt(1 - sinp^2), droll = (cr dsr - sr dcr) / (sr^2 + cr^2); residuals 2 (angle - target) / pr_var.
HuberLoss(a = 0.1) on s = |r|^2: rho = s, rho' = 1 for s <= a^2, else rho = 2 a sqrt(s) - a^2, rho' = a / sqrt(s); rho'' <= 0, so Ceres'
corrector scales residual and Jacobian by sqrt(rho'): H += rho' J^T J, g += rho' J^T r, cost += rho / 2.  Ground and IMU: NULL loss.

Factors are n x 8 doubles in rgc_mapreg_associate's layout: edge {a[3], b[3], var, valid}, plane {n[3], d, 0, 0, var, valid}.
A problem is dict(feat=[corner_cur, surf_cur, corner_last, surf_last] (n,4) float32, fac=[four (n,8)], ground=[cur, last] (dict or None),
imu=dict or None); x is q_cur t_cur q_last t_last (14)."""
import numpy as np

LD = np.longdouble
HUBER_A = LD(1) / LD(10)
E3 = np.eye(3, dtype=LD)


def _ld(a):
    return np.asarray(a, dtype=LD)


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], dtype=LD)


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]], dtype=LD)


def qrot(q, v):
    """Eigen's quaternion * vector on (..., 3)"""
    v = _ld(v)
    qv = np.broadcast_to(_ld(q)[:3], v.shape)
    u = 2 * np.cross(qv, v)
    return v + q[3] * u + np.cross(qv, u)


def quat_plus(q, d):
    d = _ld(d)
    nd = np.sqrt(np.sum(d * d))
    dq = np.concatenate([np.sin(nd) / nd * d, [np.cos(nd)]]) if nd > 0 else np.concatenate([d, [LD(1)]])
    return qmul(dq, _ld(q))


def apply_step(x, d12):
    x, d12 = _ld(x), _ld(d12)
    o = x.copy()
    for b in range(2):
        o[7 * b: 7 * b + 4] = quat_plus(x[7 * b: 7 * b + 4], d12[6 * b: 6 * b + 3])
        o[7 * b + 4: 7 * b + 7] = x[7 * b + 4: 7 * b + 7] + d12[6 * b + 3: 6 * b + 6]
    return o


def huber(s):
    """rho, rho' of HuberLoss(0.1) at the squared norms s"""
    s = _ld(s)
    out = s > HUBER_A * HUBER_A
    sq = np.sqrt(np.where(out, s, LD(1)))
    return np.where(out, 2 * HUBER_A * sq - HUBER_A * HUBER_A, s), np.where(out, HUBER_A / sq, LD(1)), out


def _dlp(Rp):
    """(n, 6, 3): the world point's differential per tangent direction"""
    n = Rp.shape[0]
    out = np.zeros((n, 6, 3), dtype=LD)
    for c in range(3):
        out[:, c] = 2 * np.cross(np.broadcast_to(E3[c], Rp.shape), Rp)
        out[:, 3 + c] = E3[c]
    return out


def edge_terms(feat, fac, q, t, baseline_scale=1):
    """valid edge factors of one set -> r (m,3), J (m,3,6), index of each in the set.  baseline_scale: |a - b| is divided by it before it
    enters s (2 = the planted error 'a 0.2 m baseline used as 0.1')"""
    idx = np.nonzero(np.asarray(fac)[:, 7] != 0)[0] if len(fac) else np.zeros(0, int)
    F = _ld(np.asarray(fac)[idx])
    p = _ld(np.asarray(feat, np.float32)[idx, :3])
    Rp = qrot(q, p)
    lp = Rp + _ld(t)
    a, b = F[:, 0:3], F[:, 3:6]
    de = a - b
    s = F[:, 6] / (np.sqrt(np.sum(de * de, axis=1)) / LD(baseline_scale))
    r = s[:, None] * np.cross(lp - a, lp - b)
    J = np.zeros((len(idx), 3, 6), dtype=LD)
    dl = _dlp(Rp)
    for c in range(6):
        J[:, :, c] = s[:, None] * np.cross(dl[:, c], de)
    return r, J, idx


def plane_terms(feat, fac, q, t):
    idx = np.nonzero(np.asarray(fac)[:, 7] != 0)[0] if len(fac) else np.zeros(0, int)
    F = _ld(np.asarray(fac)[idx])
    p = _ld(np.asarray(feat, np.float32)[idx, :3])
    Rp = qrot(q, p)
    lp = Rp + _ld(t)
    n, d, var = F[:, 0:3], F[:, 3], F[:, 6]
    r = (var * (np.sum(n * lp, axis=1) + d))[:, None]
    dl = _dlp(Rp)
    J = (var[:, None] * np.einsum("ik,ick->ic", n, dl))[:, None, :]
    return r, J, idx


def ground_terms(G, q, t):
    """r (3), J (3,6) of one Ground_DeltaFactor_goable"""
    q, t = _ld(q), _ld(t)
    ql, tl, qh = _ld(G["last_q"]), _ld(G["last_t"]), _ld(G["q_history"])
    cn, v1, v2 = _ld(G["cur_norm"]), _ld(G["last_v1"]), _ld(G["last_v2"])
    pv = LD(G.get("p_var", 0.2))
    qlc = qconj(ql)
    gn = qrot(qmul(qlc, q), cn)
    delta_t = qrot(qh, qrot(qlc, t - tl))
    a1, a2 = np.sum(v1 * gn), np.sum(v2 * gn)
    r = np.array([(LD(G["last_distance"]) - (LD(G["cur_distance"]) + delta_t[2])) / (pv / 1000), abs(a1) / (pv * 10), abs(a2) / (pv * 10)], dtype=LD)
    J = np.zeros((3, 6), dtype=LD)
    Rcn = qrot(q, cn)
    for c in range(3):
        dgn = qrot(qlc, 2 * np.cross(E3[c], Rcn))
        J[1, c] = np.sign(a1) * np.sum(v1 * dgn) / (pv * 10)
        J[2, c] = np.sign(a2) * np.sum(v2 * dgn) / (pv * 10)
        J[0, 3 + c] = -qrot(qh, qrot(qlc, E3[c]))[2] / (pv / 1000)
    return r, J, (a1, a2)


def pitch_roll(q):
    """Quaternion2EulerAngle's pitch and roll of q = x,y,z,w and their (2,3) derivative on the local parameterisation; clamped pitch: a constant"""
    q = _ld(q)
    x, y, z, w = q
    sinp = 2 * (w * y - x * z)
    sr, cr = 2 * (w * x + y * z), 1 - 2 * (x * x + y * y)
    clamped = bool(sinp >= 1 or sinp <= -1)
    pitch = (np.arccos(LD(0)) if sinp >= 1 else -np.arccos(LD(0))) if clamped else np.arcsin(sinp)
    roll = np.arctan2(sr, cr)
    D = np.zeros((2, 3), dtype=LD)
    for c in range(3):
        dx, dy, dz, dw = qmul(np.array([E3[c][0], E3[c][1], E3[c][2], 0], dtype=LD), q)
        dsinp = 2 * (dw * y + w * dy - dx * z - x * dz)
        dsr, dcr = 2 * (dw * x + w * dx + dy * z + y * dz), -4 * (x * dx + y * dy)
        D[0, c] = 0 if clamped else dsinp / np.sqrt(1 - sinp * sinp)
        D[1, c] = (cr * dsr - sr * dcr) / (sr * sr + cr * cr)
    return pitch, roll, D, clamped


def imu_terms(I, qc, ql):
    """r (7), J (7,12) of the IMU block on (q_cur, q_last)"""
    qc, ql = _ld(qc), _ld(ql)
    A = qmul(qconj(_ld(I["delta_q"])), qconj(ql))
    cov, pv = LD(I["imu_cov"]), LD(I.get("pr_var", 0.02))
    e = qmul(A, qc)
    r, J = np.zeros(7, dtype=LD), np.zeros((7, 12), dtype=LD)
    r[0:3] = 2 * e[0:3] / cov
    for c in range(3):
        de = qmul(A, qmul(np.array([E3[c][0], E3[c][1], E3[c][2], 0], dtype=LD), qc))
        J[0:3, c] = 2 * de[0:3] / cov
        J[0:3, 6 + c] = -2 * de[0:3] / cov
    pc, rc, Dc, _ = pitch_roll(qc)
    pl, rl, Dl, _ = pitch_roll(ql)
    r[3], r[4] = 2 * (pc - LD(I["pitch_cur"])) / pv, 2 * (rc - LD(I["roll_cur"])) / pv
    r[5], r[6] = 2 * (pl - LD(I["pitch_last"])) / pv, 2 * (rl - LD(I["roll_last"])) / pv
    J[3:5, 0:3] = 2 * Dc / pv
    J[5:7, 6:9] = 2 * Dl / pv
    return r, J


def _accumulate(H, g, aH, ag, r, J, w, rows):
    """+= sum_i w_i J_i^T J_i etc. for J (m, dim, cols) into the rows / columns `rows`; aH / ag take the sums of absolute values of the terms"""
    if not len(r):
        return
    ix = np.ix_(rows, rows)
    H[ix] += np.einsum("i,ika,ikc->ac", w, J, J)
    aH[ix] += np.einsum("i,ika,ikc->ac", w, np.abs(J), np.abs(J))
    g[rows] += np.einsum("i,ika,ik->a", w, J, r)
    ag[rows] += np.einsum("i,ika,ik->a", w, np.abs(J), np.abs(r))


def evaluate(prob, x, plant=None):
    """H (12,12), g (12), cost at x in longdouble, the sums of |terms| behind every entry (absH, absg; every cost term is >= 0), and per set s
    the residual norms^2, rho' and the outside-the-radius flags of its valid factors.  plant = (kind, set, i[, column]) plants one error
    (the sensitivity checks): 'drop' factor i of the set's valid ones, 'rho1' (rho' = 1 on it), 'negcol' (its Jacobian column negated),
    'baseline' (every edge factor of the set: |a - b| = 0.2 used as 0.1)."""
    x = _ld(x)
    H, g = np.zeros((12, 12), dtype=LD), np.zeros(12, dtype=LD)
    aH, ag = np.zeros((12, 12), dtype=LD), np.zeros(12, dtype=LD)
    cost = LD(0)
    per_set = []
    for s in range(4):
        b = s // 2
        q, t = x[7 * b: 7 * b + 4], x[7 * b + 4: 7 * b + 7]
        planted = plant is not None and plant[1] == s
        if s % 2 == 0:
            r, J, idx = edge_terms(prob["feat"][s], prob["fac"][s], q, t, 2 if planted and plant[0] == "baseline" else 1)
        else:
            r, J, idx = plane_terms(prob["feat"][s], prob["fac"][s], q, t)
        s2 = np.sum(r * r, axis=1) if len(r) else np.zeros(0, dtype=LD)
        rho, rho1, outer = huber(s2)
        w, cw = rho1.copy(), np.ones(len(r), dtype=LD)
        if planted and plant[0] == "drop":
            w[plant[2]] = 0
            cw[plant[2]] = 0
        if planted and plant[0] == "rho1":
            w[plant[2]] = 1
        if planted and plant[0] == "negcol":
            J = J.copy()
            J[plant[2], :, plant[3]] *= -1
        rows = np.arange(6 * b, 6 * b + 6)
        _accumulate(H, g, aH, ag, r, J, w, rows)
        cost += np.sum(cw * rho) / 2
        per_set.append(dict(index=idx, s2=s2, rho1=rho1, outer=outer, var=_ld(np.asarray(prob["fac"][s])[idx, 6]) if len(idx) else np.zeros(0, dtype=LD)))
    ground_args = [None, None]
    for b in range(2):
        G = prob["ground"][b]
        if G is not None:
            r, J, ground_args[b] = ground_terms(G, x[7 * b: 7 * b + 4], x[7 * b + 4: 7 * b + 7])
            _accumulate(H, g, aH, ag, r[None, :, None][:, :, 0], J[None], np.ones(1, dtype=LD), np.arange(6 * b, 6 * b + 6))
            cost += np.sum(r * r) / 2
    if prob["imu"] is not None:
        r, J = imu_terms(prob["imu"], x[0:4], x[7:11])
        _accumulate(H, g, aH, ag, r[None], J[None], np.ones(1, dtype=LD), np.arange(12))
        cost += np.sum(r * r) / 2
    return dict(H=H, g=g, cost=cost, absH=aH, absg=ag, sets=per_set, ground_args=ground_args)


def deviation(ref, H, g, cost):
    """the largest |difference| / sum |terms of that entry| of (H, g, cost) from the reference's, and whether every entry whose terms are all
    exactly zero is exactly zero"""
    H, g = _ld(H), _ld(g)
    dev, zeros_ok = LD(0), True
    for got, want, scale in ((H, ref["H"], ref["absH"]), (g, ref["g"], ref["absg"])):
        nz = scale > 0
        if nz.any():
            dev = max(dev, np.max(np.abs(got - want)[nz] / scale[nz]))
        zeros_ok = zeros_ok and bool(np.all(got[~nz] == 0))
    if ref["cost"] > 0:
        dev = max(dev, abs(LD(cost) - ref["cost"]) / ref["cost"])
    else:
        zeros_ok = zeros_ok and cost == 0
    return float(dev), zeros_ok


def lm_solve(prob, x0, max_iterations=6):
    """Ceres 1.14's trust-region LM as the mapping node configures it (LEVENBERG_MARQUARDT, <= 6 iterations, defaults otherwise): gradient
    tolerance 1e-10 (max norm), damping clamp(diag H, 1e-6, 1e32) / radius, initial radius 1e4, a step is accepted above a relative decrease
    of 1e-3, the radius grows by 1 / max(1/3, 1 - (2 rho - 1)^3) (<= 1e16) or shrinks by 2, 4, 8 ...; function tolerance 1e-6, parameter
    tolerance 1e-8, minimum radius 1e-32.  H, g and cost come from evaluate() (longdouble) rounded to double; the loop itself runs in double.
    Returns x, dict(iterations, successful, stop = gradient | function | parameter | radius | cap | cholesky, steps=[dict(rho, accepted, radius)], initial_cost, final_cost).  'cholesky': the
    damped system was not positive definite in the LAST iteration run (such a step counts as rejected, the loop goes on)."""
    def ev(xv):
        e = evaluate(prob, xv)
        return e["H"].astype(np.float64), e["g"].astype(np.float64), float(e["cost"])
    x = np.array(x0, dtype=np.float64)
    radius, dec = 1e4, 2.0
    H, g, cost = ev(x)
    out = dict(initial_cost=cost, successful=0, steps=[])
    it, stop = 0, "cap"
    while it < max_iterations:
        if np.abs(g).max() <= 1e-10:
            stop = "gradient"
            break
        D = np.clip(np.diag(H), 1e-6, 1e32)
        chol_failed = False
        try:
            L = np.linalg.cholesky(H + np.diag(D) / radius)
            d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
            model = float(-d @ (g + 0.5 * H @ d))
        except np.linalg.LinAlgError:
            chol_failed, model, d = True, -1.0, np.zeros(12)
        rho = -1.0
        if model > 0:
            xn = apply_step(x, d).astype(np.float64)
            Hn, gn, newc = ev(xn)
            rho = (cost - newc) / model
        it += 1
        stop = "cholesky" if chol_failed else "cap"
        if rho > 1e-3:
            old = cost
            x, H, g, cost = xn, Hn, gn, newc
            radius = min(radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 1e16)
            dec = 2.0
            out["successful"] += 1
            out["steps"].append(dict(rho=rho, accepted=True, radius=radius))
            if abs(old - cost) <= 1e-6 * old:
                stop = "function"
                break
            if np.linalg.norm(d) <= 1e-8 * (np.linalg.norm(x) + 1e-8):
                stop = "parameter"
                break
        else:
            radius /= dec
            dec *= 2.0
            out["steps"].append(dict(rho=rho, accepted=False, radius=radius))
            if radius < 1e-32:
                stop = "radius"
                break
    out.update(final_cost=cost, iterations=it, stop=stop)
    return x, out


def central_differences(prob, x, h=1e-7):
    """g and the Gauss-Newton pieces by longdouble central differences of the residuals themselves: (J_fd per set (m,dim,6), ground J (3,6) x 2, IMU J (7,12))"""
    x = _ld(x)
    h = LD(h)

    def residuals(xv):
        out = []
        for s in range(4):
            b = s // 2
            f = edge_terms if s % 2 == 0 else plane_terms
            out.append(f(prob["feat"][s], prob["fac"][s], xv[7 * b: 7 * b + 4], xv[7 * b + 4: 7 * b + 7])[0])
        for b in range(2):
            out.append(ground_terms(prob["ground"][b], xv[7 * b: 7 * b + 4], xv[7 * b + 4: 7 * b + 7])[0] if prob["ground"][b] is not None else None)
        out.append(imu_terms(prob["imu"], xv[0:4], xv[7:11])[0] if prob["imu"] is not None else None)
        return out
    cols = []
    for a in range(12):
        d = np.zeros(12, dtype=LD)
        d[a] = h
        rp, rm = residuals(apply_step(x, d)), residuals(apply_step(x, -d))
        cols.append([None if p is None else (p - m) / (2 * h) for p, m in zip(rp, rm)])
    sets = [np.stack([cols[6 * (s // 2) + c][s] for c in range(6)], axis=-1) for s in range(4)]
    ground = [None if cols[0][4 + b] is None else np.stack([cols[6 * b + c][4 + b] for c in range(6)], axis=-1) for b in range(2)]
    imu = None if cols[0][6] is None else np.stack([cols[a][6] for a in range(12)], axis=-1)
    return sets, ground, imu
