"""The reference's view of a designed sweep (tests/fe_cases.py): the literal Python restatement (oracle/py_frontend.py) run stage by
stage, the C oracle's outputs next to it, and a CENSUS of the branches the sweep makes the reference take.  Nothing here touches the
product: a census minimum that holds proves, on the CPU, that the sweep drives the selection / stencil / bucket code into the branch
it was designed for -- the GPU test then only has to hold the product to the oracle on that sweep.
"""
import numpy as np

import fe_cases
from oracle import py_frontend as pf

f32 = np.float32
_memo = {}


def a1_filter(raw, min_range=0.5, max_range=80.0):
    """:112-113, :732-763 restated: NaN, squared range in float against the two thresholds, the strip behind the sensor"""
    raw = np.asarray(raw, f32)
    x, y, z = raw[:, 0], raw[:, 1], raw[:, 2]
    with np.errstate(invalid="ignore"):
        dis = (x * x + y * y) + z * z
        keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~(dis < f32(min_range) * f32(min_range)) & ~(dis > f32(max_range) * f32(max_range)) \
            & ~((x < 0) & (np.abs(y) < f32(0.5)))
    return keep


def restate(raw, prm):
    """the Python restatement, stage by stage; None for an empty sweep"""
    keep = a1_filter(raw)
    if not keep.any():
        return None
    ns = prm["n_scans"]
    rb = pf.ring_bucket(raw[keep], ns)
    if len(rb["cloud"]) == 0:
        return None
    st = pf.stencils(rb["cloud"][:, :3], rb["intensity_num"])
    occ = pf.occlusion(st["range"])
    mark, pushed, gp = pf.ground(rb["cloud"], rb["ring_count"], st["range"])
    trace = []
    sel = pf.select(rb["cloud"], st, occ, mark, rb["scan_start"], rb["scan_end"], prm.get("use_intensity", 1), trace=trace)
    return dict(keep=keep, rb=rb, st=st, occ=occ, mark=mark, pushed=pushed, gp=gp, sel=sel, trace=trace)


def pin(o, r):
    """the C oracle against the restatement on the keys tests/fuzz/fuzz_oracle_pin_frontend.py compares: bit for bit, the ground plane
    within that pin's bounds where the plane is determined.  Returns the list of differing keys."""
    bad = []
    rb, st, sel = r["rb"], r["st"], r["sel"]
    ns = len(rb["ring_count"])
    if rb["cloud"].shape != o["cloud"].shape or not np.array_equal(rb["cloud"], o["cloud"]):
        return ["A2 cloud"]
    for k in ("ring_count", "scan_start", "scan_end"):
        if not np.array_equal(rb[k], o[k][:ns]):
            bad.append(k)
    for k in ("curvature", "curvature2", "inten_curvature"):
        if not np.array_equal(st[k], o[k], equal_nan=True):
            bad.append(k)
    if not np.array_equal(r["mark"], o["ground_marked"]):
        bad.append("ground_marked")
    if len(r["pushed"]) != len(o["ground_pts"]) or not np.array_equal(o["ground_pts"][:, :3], o["cloud"][r["pushed"], :3]):
        bad.append("ground_pts")
    if (r["gp"] is not None) != bool(o["ground_valid"]):
        bad.append("ground_valid")
    elif r["gp"] is not None:
        go, g = np.asarray(o["groundparam"]), r["gp"]
        if ground_determined(o["ground_pts"][:, :3]):                     # judged on the ORACLE's ground set
            if not (np.abs(go[0:3] - g[0:3]).max() < 1e-7 and abs(go[9] - g[9]) < 1e-8 and abs(go[10] - g[10]) < 1e-8):
                bad.append("groundparam")
        elif len(o["ground_pts"]) > 30:
            # no plane in the set: the normal is not determined, nor is distance unless both sides chose the same normal; 1 - src1 is
            if not abs(go[10] - g[10]) < 1e-8:
                bad.append("groundparam 1 - src1")
            if np.abs(go[0:3] - g[0:3]).max() < 1e-7 and not abs(go[9] - g[9]) < 1e-8:
                bad.append("groundparam distance")
            if not (abs(np.linalg.norm(go[0:3]) - 1) < 1e-9 and np.isfinite(go).all()):
                bad.append("groundparam normal not a unit vector")
    for k in ("label", "inten_label", "picked"):
        if not np.array_equal(sel[k], o[k]):
            bad.append(k)
    if sel["n_sharp_own"] != o["n_sharp_own"]:
        bad.append("n_sharp_own")
    for k in ("sharp", "flat", "inten"):
        if sel[k].shape != o[k].shape or not np.array_equal(sel[k], o[k]):
            bad.append(k)
    return bad


def ground_determined(pts):
    """the weighted plane fit has a direction to find: the two smallest eigenvalues of the ground set's covariance are apart (the pin's
    test).  Otherwise the smallest eigenvector -- the normal -- is arbitrary within a plane (a collinear set) or altogether (one repeated
    point), and so is `distance` = the mean of normal . p; `1 - src1` is still determined (every offset is along the line or zero)."""
    pts = np.asarray(pts, np.float64)
    if len(pts) <= 30:
        return False
    ev = np.linalg.eigvalsh(np.cov(pts.T))
    return bool(ev[1] > 1e3 * max(ev[0], 1e-12))


def _tied(keys, ok, sectors):
    """candidates that pass a pass's static test and share their key with another such candidate of the same sector"""
    n = 0
    for sp, ep in sectors:
        idx = np.arange(sp, ep + 1)[ok[sp:ep + 1]]
        if len(idx) > 1:
            _, inv, cnt = np.unique(keys[idx], return_inverse=True, return_counts=True)
            n += int(np.sum(cnt[inv] > 1))
    return n


def census(name):
    """counts of what the reference does on a case, from the restatement alone (memoised)"""
    if name in _memo:
        return _memo[name]
    raw, prm, _ = fe_cases.get(name)
    r = restate(raw, prm)
    keep = a1_filter(raw)
    kept = np.flatnonzero(keep)
    c = dict(empty=int(r is None), n_raw=len(raw))
    if len(kept):
        c.update({"first_lane_%d" % (kept[0] % 64): 1, "last_lane_%d" % (kept[-1] % 64): 1})
    if r is None:
        _memo[name] = (c, r)
        return c, r
    rb, st, sel, occ = r["rb"], r["st"], r["sel"], r["occ"]
    n = len(rb["cloud"])
    rc = rb["ring_count"]
    starts = np.concatenate([[0], np.cumsum(rc)])
    rng, ang, icv, cv, cv2 = st["range"], st["angle"], st["inten_curvature"], st["curvature"], st["curvature2"]
    inner = np.zeros(n, bool)
    inner[5:n - 5] = True
    near = inner & (rng < 2)
    c.update(n_cloud=n, outside_fan=int(keep.sum()) - n, max_ring=int(rc.max()), rings_in_use=int(np.count_nonzero(rc)),
             near=int(near.sum()), near_gate=int(np.sum(near & (ang < 0.07))), near_no_gate=int(np.sum(near & ~(ang < 0.07))),
             smoothed=int(np.sum(st["intensity_num"] != rb["intensity_num"])),
             near_inten_features=int(np.sum((sel["inten_label"] == 2) & near & (ang < 0.07))),
             range_eq_2=int(np.sum(inner & (rng == f32(2)))), range_below_2=int(np.sum(inner & (rng == np.nextafter(f32(2), f32(0))))),
             range_above_2=int(np.sum(inner & (rng == np.nextafter(f32(2), f32(3))))))
    for m in (19, 20, 21, 81, 82):
        c["ring_%d" % m] = int(np.sum(rc == m))
    c["group_%d" % fe_cases.staging_group(c["max_ring"])] = 1
    sectors, ring_of_sector = [], []
    for i in range(len(rc)):
        if rb["scan_end"][i] - rb["scan_start"][i] >= 10:
            b = fe_cases.sector_bounds(int(starts[i]), int(rc[i]))
            sectors += b
            ring_of_sector += [i] * 6
    c["max_sector"] = max([ep - sp + 1 for sp, ep in sectors], default=0)
    c["parallel_rings"] = sum(1 for i in range(len(rc)) if rb["scan_end"][i] - rb["scan_start"][i] >= 10
                              and min(ep - sp + 1 for sp, ep in fe_cases.sector_bounds(int(starts[i]), int(rc[i]))) >= 12)
    c["ring_start_tiles"] = int(np.sum([(s % 256) in (0, 5, 10, 246, 251) for s in starts[1:len(rc)] if s < n]))
    # quotas: the counters the three loops leave behind (22 / 41 / 22: a further candidate met the quota's `break`)
    ks = np.array([t[2] for t in r["trace"]]).reshape(-1, 3)
    c.update(sharp_label_1=int(np.sum(ks[:, 0] >= 21)), sharp_quota_cut=int(np.sum(ks[:, 0] == 22)), flat_quota_cut=int(np.sum(ks[:, 1] == 41)),
             inten_label_1=int(np.sum(ks[:, 2] >= 21)), inten_quota_cut=int(np.sum(ks[:, 2] == 22)))
    nf, ns_own, ni = len(sel["flat"]), sel["n_sharp_own"], len(sel["inten"])
    added = bool(prm.get("use_intensity", 1)) and nf > 0 and ns_own / nf < 0.3
    c.update(n_flat_zero=int(nf == 0), add_inten=int(added and ni > 0), inten_found_not_added=int(ni > 0 and not added),
             ratio_ge_03_with_flat=int(nf > 0 and ni > 0 and ns_own / nf >= 0.3), ratio=(ns_own / nf if nf else float("inf")))
    # ties among the candidates that pass each pass's static test (flags as the passes find them at the sector's start do not enter)
    gm = r["mark"] == 1
    c.update(tied_sharp=_tied(cv, ~gm & (cv > 0.1) & (cv2 > 0.3), sectors), tied_flat=_tied(cv, (cv < 0.3) & (cv2 < 0.4), sectors),
             tied_inten=_tied(icv, ~gm & (icv > 65), sectors))
    rev = pf.select(rb["cloud"], st, occ, r["mark"], rb["scan_start"], rb["scan_end"], prm.get("use_intensity", 1), tie=-1)
    differs = (rev["label"] != sel["label"]) | (rev["inten_label"] != sel["inten_label"])
    c["tie_order_decides"] = sum(1 for sp, ep in sectors if differs[sp:ep + 1].any())
    # start-over: a sector run alone (on the flags as the occlusion pass left them) against the same sector of the serial walk
    redo_label = redo_inten_only = 0
    if n <= 4000:
        for (sp, ep), i in zip(sectors, ring_of_sector):
            j = [b for b in fe_cases.sector_bounds(int(starts[i]), int(rc[i]))].index((sp, ep))
            if j == 0:
                continue
            alone = pf.select(rb["cloud"], st, occ, r["mark"], rb["scan_start"], rb["scan_end"], prm.get("use_intensity", 1), only=(i, j))
            dl = not np.array_equal(alone["label"][sp:ep + 1], sel["label"][sp:ep + 1])
            di = not np.array_equal(alone["inten_label"][sp:ep + 1], sel["inten_label"][sp:ep + 1])
            redo_label += dl
            redo_inten_only += (di and not dl)
    c.update(redo_label=redo_label, redo_inten_only=redo_inten_only)
    # thresholds
    num = st["intensity_num"]
    dnum = np.abs(np.diff(num))
    pick = sel["inten_label"] == 2
    next_to_pick = pick[:-1] | pick[1:]
    c.update(icurv_64=int(np.sum(inner & (icv == 64))), icurv_65=int(np.sum(inner & (icv == 65))), icurv_66=int(np.sum(inner & (icv == 66))),
             step_35=int(np.sum((dnum == 35) & next_to_pick)), step_36=int(np.sum((dnum == 36) & next_to_pick)))
    P = rb["cloud"][:, :3]
    d = P[1:] - P[:-1]
    gap = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    c.update(gap_below=int(np.sum((gap > 0.045) & (gap <= 0.05))), gap_above=int(np.sum((gap > 0.05) & (gap < 0.055))))
    d1, d2 = rng[5:n - 6].astype(np.float64), rng[6:n - 5].astype(np.float64)
    ratio = np.abs(d1 - d2) / np.minimum(d1, d2)
    c["occl_near_004"] = int(np.sum(np.abs(ratio - 0.04) < 2e-4))
    i_last = n - 6
    c["occl_mark_at_cs"] = int(n > 12 and f32(rng[i_last + 1] - rng[i_last]) > 0.04 * float(rng[i_last]) and not f32(rng[i_last] - rng[i_last + 1]) > 0.04 * float(rng[i_last + 1]))
    cross = 0
    for i in range(5, n - 5):
        a, b = rng[i], rng[i + 1]
        lo_hi = (i - 5, i) if f32(a - b) > 0.04 * float(b) else (i + 1, i + 6) if f32(b - a) > 0.04 * float(a) else None
        if lo_hi and np.any((starts[1:len(rc)] > lo_hi[0]) & (starts[1:len(rc)] <= lo_hi[1])):
            cross += 1
    c["occl_cross_ring"] = cross
    # ground
    gpts = rb["cloud"][r["pushed"], :3]
    c.update(no_ground=int(len(r["pushed"]) == 0), ground_pts=len(r["pushed"]), ground_degenerate=int(len(gpts) > 30 and not ground_determined(gpts)))
    # the curvature thresholds: candidates within 1e-7 (curvature) / 5e-6 (curvature2) of each, by the side of the comparison they are on,
    # counted only where the other conditions of the pass hold and the label is what this comparison alone decides
    lab = sel["label"]
    free = inner & (r["mark"] != 1) & (occ == 0)
    near_ = lambda v, t, d: np.abs(v.astype(np.float64) - t) <= d
    c.update(curv_01_hi=int(np.sum(free & near_(cv, 0.1, 1e-7) & (cv > 0.1) & (cv2 > 0.3) & (lab == 2))),
             curv_01_lo=int(np.sum(free & near_(cv, 0.1, 1e-7) & ~(cv > 0.1) & (cv2 > 0.3) & (lab != 2))),
             curv_03_lo=int(np.sum(free & near_(cv, 0.3, 1e-7) & (cv < 0.3) & (cv2 < 0.3) & (lab == -1))),
             curv_03_hi=int(np.sum(free & near_(cv, 0.3, 1e-7) & ~(cv < 0.3) & (cv2 < 0.3) & (lab == 0))),
             curv2_03_hi=int(np.sum(free & near_(cv2, 0.3, 5e-6) & (cv2 > 0.3) & (cv > 0.1) & (cv < 0.3) & (lab == 2))),
             curv2_03_lo=int(np.sum(free & near_(cv2, 0.3, 5e-6) & ~(cv2 > 0.3) & (cv > 0.1) & (cv < 0.3) & (lab == -1))),
             curv2_04_lo=int(np.sum(free & near_(cv2, 0.4, 5e-6) & (cv2 < 0.4) & (cv < 0.1) & (lab == -1))),
             curv2_04_hi=int(np.sum(free & near_(cv2, 0.4, 5e-6) & ~(cv2 < 0.4) & (cv < 0.1) & (lab == 0))),
             curv_01_adjacent=int(np.sum(cv == f32(0.1)) > 0 and np.sum(cv == np.nextafter(f32(0.1), f32(0))) > 0),
             curv_03_adjacent=int(np.sum(cv == f32(0.3)) > 0 and np.sum(cv == np.nextafter(f32(0.3), f32(0))) > 0))
    _memo[name] = (c, r)
    return c, r
