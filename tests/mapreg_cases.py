"""Designed problems for the mapping node's feature-registration solve (f1): what tests/test_mapreg_reference.py (no GPU) and
tests/test_gpu_mapreg_terms.py run.  Designed geometry, not the synthetic front-end's scenes: the maps are lattice-like samples (0.4 m, jittered
in the plane only, so no two map points tie in distance) of a floor at z = -1.5, four walls at |x|, |y| = 8 and eight vertical poles
(0.2 m in z), which keeps the association far from its thresholds (tested in test_gpu_association.py); the features are samples of the same
structures seen from the true poses, with Gaussian noise, planted outliers and per-feature weights.

Every case declares MINIMA that test_mapreg_reference.py asserts from the longdouble reference alone (census()), so a case cannot quietly stop
covering what it was built for.  LM-path cases were found by searching seeds and perturbation sizes on the CPU (the C oracle and the
reference's restatement of the loop must both take the path); PATHS_NOT_BUILT names what the search did not find."""
import functools

import numpy as np

import mapreg_reference as ref

FLOOR_Z, WALL, POLES = -1.5, 8.0, [(3.0, 2.0), (-2.5, 3.5), (4.0, -3.0), (-3.5, -2.5), (0.5, 5.0), (5.5, 0.5), (-5.0, 0.0), (0.0, -5.5)]


@functools.lru_cache(maxsize=None)
def maps():
    """(corner_map (1048,3), surf_map (3003,3)) float32"""
    rng = np.random.default_rng(11)
    g = np.arange(-WALL, WALL + 1e-9, 0.4)
    X, Y = np.meshgrid(g, g)
    floor = np.stack([X.ravel(), Y.ravel(), np.full(X.size, FLOOR_Z)], 1)
    floor[:, :2] += rng.uniform(-0.05, 0.05, (len(floor), 2))
    zs = np.arange(FLOOR_Z + 0.4, 1.5, 0.4)
    A, Z = np.meshgrid(g, zs)
    walls = []
    for axis in (0, 1):
        for sgn in (-1.0, 1.0):
            w = np.zeros((A.size, 3))
            w[:, axis], w[:, 1 - axis], w[:, 2] = sgn * WALL, A.ravel(), Z.ravel()
            w[:, 1 - axis] += rng.uniform(-0.05, 0.05, len(w))
            w[:, 2] += rng.uniform(-0.05, 0.05, len(w))
            walls.append(w)
    pz = np.arange(FLOOR_Z, 2.5 + 1e-9, 0.2)
    poles = []
    for (px, py) in POLES:
        p = np.stack([np.full(len(pz), px), np.full(len(pz), py), pz + rng.uniform(-0.03, 0.03, len(pz))], 1)
        p[:, :2] += rng.normal(0, 0.002, (len(pz), 2))
        poles.append(p)
    corner = np.concatenate(poles).astype(np.float32)
    return corner, np.concatenate([floor] + walls).astype(np.float32)


def quat(rotvec):
    r = np.asarray(rotvec, float)
    th = np.linalg.norm(r)
    return np.concatenate([np.sin(th / 2) * r / th, [np.cos(th / 2)]]) if th > 0 else np.array([0.0, 0.0, 0.0, 1.0])


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def sample(rng, q, t, n_corner, n_surf, noise=0.02, out_corner=0, out_surf=0, floor_only=False, weights="vary"):
    """features (n,4) float32 {x, y, z, weight} in the sensor frame of the pose (q, t): corners on the poles, surfs on the floor and the walls.
    The first out_* of each kind are outliers: 0.25 .. 0.45 m off their structure (beyond the Huber radius at any weight >= 0.5)."""
    R = _rot(q)
    def finish(w_pts, n_out, normal):
        off = rng.normal(0, noise, (len(w_pts), 1)) * normal
        off[:n_out] = (rng.uniform(0.25, 0.45, (n_out, 1)) * rng.choice([-1.0, 1.0], (n_out, 1))) * normal[:n_out]
        body = (w_pts + off - t) @ R                     # R^T (p - t)
        w = rng.uniform(0.5, 1.5, len(body)) if weights == "vary" else np.ones(len(body))
        return np.concatenate([body, w[:, None]], 1).astype(np.float32).reshape(-1, 4)
    pole = rng.integers(0, len(POLES), n_corner)
    cw = np.stack([np.array(POLES)[pole, 0], np.array(POLES)[pole, 1], rng.uniform(FLOOR_Z + 0.6, 1.8, n_corner)], 1) if n_corner else np.zeros((0, 3))
    ang = rng.uniform(0, 2 * np.pi, n_corner)
    corner = finish(cw, out_corner, np.stack([np.cos(ang), np.sin(ang), np.zeros(n_corner)], 1) if n_corner else np.zeros((0, 3)))
    on_floor = np.ones(n_surf, bool) if floor_only else rng.random(n_surf) < 0.6
    sw, sn = np.zeros((n_surf, 3)), np.zeros((n_surf, 3))
    for i in range(n_surf):
        if on_floor[i]:
            sw[i], sn[i] = [rng.uniform(-5, 5), rng.uniform(-5, 5), FLOOR_Z], [0, 0, 1]
        else:
            axis, sgn = rng.integers(0, 2), rng.choice([-1.0, 1.0])
            sw[i, axis], sw[i, 1 - axis], sw[i, 2] = sgn * WALL, rng.uniform(-6, 6), rng.uniform(FLOOR_Z + 0.9, 0.6)
            sn[i, axis] = 1
    return corner, finish(sw, out_surf, sn)


def perturbed(rng, x, ang, trans):
    """x (14) with both poses moved: a rotation of about `ang` rad applied on the left, a translation of about `trans` m"""
    o = np.array(x, float)
    for b in range(2):
        o[7 * b: 7 * b + 4] = np.asarray(ref.qmul(ref._ld(quat(rng.normal(0, ang, 3))), ref._ld(x[7 * b: 7 * b + 4])), float)
        o[7 * b + 4: 7 * b + 7] += rng.normal(0, trans, 3)
    return o


def make_ground(q, t, q_last, t_last, s1, s2, p_var=0.2):
    """a Ground_DeltaFactor_goable whose two |.| arguments are s1 * 0.02 and s2 * 0.02 at the pose (q, t): away from the kink by far more than
    any step of a finite difference, with the chosen signs"""
    Rl, Rc = _rot(q_last), _rot(q)
    n_l = Rl.T @ np.array([0.0, 0.0, 1.0])
    v1 = np.cross(n_l, [1.0, 0.0, 0.0]); v1 /= np.linalg.norm(v1)
    v2 = np.cross(n_l, v1)
    gn = n_l + 0.02 * s1 * v1 + 0.02 * s2 * v2
    gn /= np.linalg.norm(gn)
    cn = Rc.T @ (Rl @ gn)                                   # q_last* (q cn) = gn
    h_l, h_c = t_last[2] - FLOOR_Z, t[2] - FLOOR_Z
    return dict(last_v1=v1, last_v2=v2, last_norm=n_l, last_distance=h_l, cur_norm=cn, cur_distance=h_c + 0.004, q_history=np.array(q_last, float),
                last_q=np.array(q_last, float), last_t=np.array(t_last, float), p_var=p_var)


def make_imu(q, q_last, imu_cov, pr_var=0.02):
    dq = np.asarray(ref.qmul(ref._ld(quat([0.002, -0.001, 0.0015])), ref.qmul(ref.qconj(ref._ld(q_last)), ref._ld(q))), float)
    pc, rc = (float(v) for v in ref.pitch_roll(q)[:2])
    pl, rl = (float(v) for v in ref.pitch_roll(q_last)[:2])
    return dict(delta_q=dq, imu_cov=imu_cov, pitch_cur=pc + 0.004, roll_cur=rc - 0.003, pitch_last=pl + 0.002, roll_last=rl - 0.004, pr_var=pr_var)


X_TRUE = np.concatenate([quat([0.01, -0.02, 0.05]), [0.30, -0.20, 0.05], quat([-0.015, 0.01, 0.03]), [0.10, 0.15, 0.02]])

# name: (seed, (n_corner_cur, n_surf_cur, n_corner_last, n_surf_last), keyword options)
#   outliers: planted per set; ang / trans: the start's distance from the truth; ground: the signs (s1, s2) of the two poses' blocks; imu: imu_cov;
#   lm: part of the rgc_mapreg_optimize comparison (the gate of :1069 needs > 10 corners and > 50 surfs in the current pose);
#   minima: what census() must show at least (asserted without a GPU); path: the LM path the case exists for
SPECS = {
    "huber":        (1, (300, 800, 260, 700), dict(outliers=40, near_radius=True, zero_weight=True, lm=True,
                                                  minima=dict(inside=20, outside=20, near_radius=1, zero_weight=1, blocks=(5, 4)))),
    "smallest":     (2, (11, 51, 11, 51), dict(lm=True, minima=dict(blocks=(1, 1)))),
    "n255":         (3, (37, 218, 0, 100), dict(outliers=5, lm=True, minima=dict(total_cur=255, blocks=(1, 1), edge_plane_split_inside_wave=True))),
    "n256":         (4, (37, 219, 50, 0), dict(outliers=5, lm=True, minima=dict(total_cur=256, blocks=(1, 1), edge_plane_split_inside_wave=True))),
    "n257":         (5, (37, 220, 0, 0), dict(outliers=5, lm=True, minima=dict(total_cur=257, blocks=(2, 0), edge_plane_split_inside_wave=True))),
    "n513":         (6, (101, 412, 30, 100), dict(outliers=8, lm=True, minima=dict(total_cur=513, blocks=(3, 1), edge_plane_split_inside_wave=True))),
    "blocks_1_3":   (7, (30, 100, 101, 412), dict(outliers=8, lm=True, minima=dict(blocks=(1, 3)))),
    "all_invalid":  (8, (11, 51, 11, 51), dict(far=True, lm=True, scale_q=1.5, minima=dict(no_factors=True), path="gradient")),
    "planes_ez":    (9, (11, 200, 0, 150), dict(far_corners=True, floor_only=True, minima=dict(planes_ez=True))),
    "ground_pp_mm": (10, (60, 200, 50, 180), dict(outliers=6, ground=((1, 1), (-1, -1)), minima=dict(ground_signs=((1, 1), (-1, -1))))),
    "ground_pm_mp": (11, (60, 200, 50, 180), dict(outliers=6, ground=((1, -1), (-1, 1)), minima=dict(ground_signs=((1, -1), (-1, 1))))),
    "imu_0.4":      (12, (60, 200, 50, 180), dict(outliers=6, imu=0.4, minima=dict(imu=True))),
    "imu_0.004":    (13, (60, 200, 50, 180), dict(outliers=6, imu=0.004, minima=dict(imu=True))),
    "ground_imu":   (14, (60, 200, 50, 180), dict(outliers=6, imu=0.4, ground=((1, -1), (1, 1)), minima=dict(imu=True, ground_signs=((1, -1), (1, 1))))),
}
# the LM path each pass of the two-pass loop must take in these cases: (stop reason, a rejected step followed by an accepted one)
PATHS = {"lm_rejected_cap": (("cap", True), ("function", False)), "lm_function": (("function", False), ("function", False)),
         "lm_function_at_6": (("function", False), ("function", False)), "all_invalid": (("gradient", False), ("gradient", False))}
# a stop on parameter tolerance was not built: |step| <= 1e-8 (|x| + 1e-8) with a relative cost change still above 1e-6 (function tolerance is
# tested first) needs a start within about 1e-8 of a minimum of nearly zero cost; no (seed, perturbation) of the search reached it
PATHS_NOT_BUILT = ["parameter"]


def lm_spec(seed, n, ang, trans, outliers, path):
    return (seed, n, dict(outliers=outliers, ang=ang, trans=trans, lm=True, path=path, minima=dict(path=path)))


# found by searching seeds x perturbation sizes on the CPU (EXPERIMENTS.md): both the C oracle and the reference's restatement take the path,
# and an independent association (oracle/py_mapreg.py) decides every feature as the oracle does at the poses of both passes
SPECS["lm_function"] = lm_spec(100, (100, 400, 80, 300), 0.004, 0.03, 10, "function")
SPECS["lm_function_at_6"] = lm_spec(102, (100, 400, 80, 300), 0.08, 0.03, 10, "function")     # the sixth step meets the tolerance: it++ and break at the cap
SPECS["lm_rejected_cap"] = lm_spec(104, (11, 51, 11, 51), 0.4, 0.1, 3, "rejected")             # pass 1: three steps rejected, then three accepted, stop at the cap
LM_CASES = [n for n, sp in SPECS.items() if sp[2].get("lm")]
# planes_ez is NOT among them: x, y and yaw are unobservable, the solve rests on the 1e-6 / radius damping, and at the converged second pass the
# step's actual cost change is rounding noise -- the reference's restatement rejects six steps where the C oracle accepts one (poses 1.2e-5
# apart, costs equal to 3e-16).  Its read-out is asserted, its LM is not (the ground and IMU cases: the existing tests of test_gpu_mapreg.py)

# the largest |oracle - reference| / sum |terms| over all cases at x0 and x_eval, measured on the CPU (test_mapreg_reference.py keeps it current;
# EXPERIMENTS.md): the C oracle is the same formulas in plain sequential fp64, and a tree-ordered sum may differ from it by a small multiple.
# With a ground or IMU block the figure is the truncation and rounding of the blocks' central-difference Jacobians (step 1e-6), which the
# library and the oracle share; without one it is fp64 rounding alone, and those cases are held to the tighter bar.
DEV_ALL, DEV_FEATURES = 2.0e-10, 1.2e-14
BAR, BAR_FEATURES = 8 * DEV_ALL, 8 * DEV_FEATURES


# Shapes of the term kernel's block sums and of the fold (256 factors per workgroup, one wave per column striding 64 rows), for the GPU read-out only:
# one factor (one lane), 63 (a partial wave), 257 (n257 above: a second workgroup of one lane) and 16500 in the current pose (65 partial rows: the
# fold's second stride).  Not in SPECS: the tests without a GPU and their recorded figures run over SPECS and stay what they are.
SHAPE_SPECS = {
    "shape_1":     (21, (0, 1, 0, 0), dict(minima={})),
    "shape_63":    (22, (12, 51, 0, 0), dict(outliers=3, minima={})),
    "shape_16500": (23, (4000, 12500, 30, 100), dict(outliers=40, minima={})),
}


def bar_of(case):
    return BAR if (case["imu"] is not None or case["ground"][0] is not None or case["ground"][1] is not None) else BAR_FEATURES


@functools.lru_cache(maxsize=None)
def build(name):
    seed, n, opt = SPECS[name] if name in SPECS else SHAPE_SPECS[name]
    rng = np.random.default_rng(1000 + seed)
    corner_map, surf_map = maps()
    xt = X_TRUE.copy()
    n_out = opt.get("outliers", 0)
    feats = []
    for b in range(2):
        q, t = xt[7 * b: 7 * b + 4], xt[7 * b + 4: 7 * b + 7]
        nc, ns = n[2 * b], n[2 * b + 1]
        c, s = sample(rng, q, t, nc, ns, out_corner=min(n_out, nc // 3), out_surf=min(n_out, ns // 3), floor_only=opt.get("floor_only", False))
        if opt.get("far"):
            c[:, :3] += np.float32(100.0)
            s[:, :3] += np.float32(100.0)
        if opt.get("far_corners"):
            c[:, :3] += np.float32(100.0)
        feats += [c, s]
    x0 = perturbed(rng, xt, opt.get("ang", 0.004), opt.get("trans", 0.03))
    if opt.get("scale_q"):
        x0[0:4] *= opt["scale_q"]
        x0[7:11] *= 0.5
    ground = [None, None]
    if opt.get("ground"):
        ground = [make_ground(xt[7 * b: 7 * b + 4], xt[7 * b + 4: 7 * b + 7], xt[7:11], xt[11:14] if b == 0 else xt[11:14] - [0.2, 0.1, 0.0], *opt["ground"][b]) for b in range(2)]
    imu = make_imu(xt[0:4], xt[7:11], opt["imu"]) if opt.get("imu") else None
    if opt.get("zero_weight"):
        for s in range(4):
            feats[s][len(feats[s]) // 2, 3] = 0.0
    if opt.get("near_radius"):
        _tune_near_radius(feats, corner_map, surf_map, x0)
    x_eval = perturbed(np.random.default_rng(2000 + seed), x0, 0.002, 0.01)   # a second pose for the frozen factors
    return dict(name=name, corner_map=corner_map, surf_map=surf_map, feat=feats, ground=ground, imu=imu, x0=x0, x_eval=x_eval, x_true=xt,
                lm=bool(opt.get("lm")), minima=opt["minima"], path=opt.get("path"))


def associate(case, x):
    """the four factor sets (n,8) of the case at x from the C oracle (the layout of rgc_mapreg_associate)"""
    from oracle import oracle
    out = []
    for s in range(4):
        b = s // 2
        mp = case["corner_map"] if s % 2 == 0 else case["surf_map"]
        out.append(factors8(oracle.mapreg_associate(case["feat"][s], x[7 * b: 7 * b + 4], x[7 * b + 4: 7 * b + 7], mp, "edge" if s % 2 == 0 else "plane"),
                            "edge" if s % 2 == 0 else "plane"))
    return out


def factors8(f, kind):
    n = len(f["valid"])
    F = np.zeros((n, 8))
    if n:
        if kind == "edge":
            F[:, 0:3], F[:, 3:6] = f["a"], f["b"]
        else:
            F[:, 0:3], F[:, 3] = f["n"], f["d"]
        F[:, 6], F[:, 7] = f["var"], f["valid"]
        F[~np.asarray(f["valid"], bool)] = 0.0
    return F


def factor_dict(F, kind):
    """the inverse of factors8: what oracle.make_factors takes"""
    F = np.asarray(F).reshape(-1, 8)
    if kind == "edge":
        return dict(valid=F[:, 7] != 0, a=F[:, 0:3], b=F[:, 3:6], var=F[:, 6])
    return dict(valid=F[:, 7] != 0, n=F[:, 0:3], d=F[:, 3], var=F[:, 6])


def oracle_evaluate(case, fac, x):
    """H, g, cost of the C oracle (orc_mapreg_evaluate) on the frozen factors fac at x"""
    from oracle import oracle
    kinds = ("edge", "plane", "edge", "plane")
    raw = [oracle.make_factors(factor_dict(fac[s], kinds[s]), kinds[s]) for s in range(4)]
    f = case["feat"]
    return oracle.mapreg_evaluate(f[0], raw[0], f[1], raw[1], f[2], raw[2], f[3], raw[3], x, ground_cur=case["ground"][0], ground_last=case["ground"][1],
                                  imu=case["imu"])


def oracle_optimize(case):
    from oracle import oracle
    f = case["feat"]
    return oracle.mapreg_optimize(f[0], f[1], f[2], f[3], case["corner_map"], case["surf_map"], case["x0"], ground_cur=case["ground"][0],
                                  ground_last=case["ground"][1], imu=case["imu"])


def problem(case, fac):
    return dict(feat=case["feat"], fac=fac, ground=case["ground"], imu=case["imu"])


def _tune_near_radius(feats, corner_map, surf_map, x0):
    """per set, two inliers' weights are set so that the residual norm is the Huber radius 0.1 -+ 5e-7 at x0 (the weight is a float32 near 1: steps
    of 1e-8 in the residual).  Their distances to the structure are raised to about 0.1 m first, through the weight alone: r = weight * distance."""
    case = dict(corner_map=corner_map, surf_map=surf_map, feat=feats)
    for s in range(4):
        feats[s][-2:, 3] = 1.0
    fac = associate(case, x0)
    e = ref.evaluate(dict(feat=feats, fac=fac, ground=[None, None], imu=None), x0)
    for s in range(4):
        st = e["sets"][s]
        for k, target in ((len(feats[s]) - 2, 0.1 - 5e-7), (len(feats[s]) - 1, 0.1 + 5e-7)):
            pos = np.nonzero(st["index"] == k)[0]
            assert len(pos) == 1, "the tuned feature must have a factor"
            dist = float(np.sqrt(st["s2"][pos[0]]))
            feats[s][k, 3] = np.float32(target / dist)


def census(case, fac, x):
    """what the case covers at x, from the reference alone: per set the factor count and the counts strictly inside / outside the Huber radius,
    within 1e-6 of it on either side, valid factors of weight 0; feature counts and blocks of 256 per pose; the signs of the ground blocks' |.|
    arguments"""
    e = ref.evaluate(problem(case, fac), x)
    out = dict(sets=[], blocks=tuple(-(-(len(case["feat"][2 * b]) + len(case["feat"][2 * b + 1])) // 256) for b in range(2)),
               n_feat=tuple(len(f) for f in case["feat"]))
    for s in range(4):
        st = e["sets"][s]
        r = np.sqrt(st["s2"]).astype(np.float64) if len(st["s2"]) else np.zeros(0)
        out["sets"].append(dict(factors=len(r), inside=int((r < 0.1).sum()), outside=int((r > 0.1).sum()),
                                just_inside=int(((r < 0.1) & (r > 0.1 - 1e-6)).sum()), just_outside=int(((r > 0.1) & (r < 0.1 + 1e-6)).sum()),
                                zero_weight=int((st["var"] == 0).sum())))
    out["ground_signs"] = tuple(None if a is None else (int(np.sign(a[0])), int(np.sign(a[1]))) for a in e["ground_args"])
    out["ground_margin"] = min([float(min(abs(a[0]), abs(a[1]))) for a in e["ground_args"] if a is not None], default=None)
    return out
