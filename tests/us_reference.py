"""An independent numpy reference for pcl::UniformSampling and the mapping node's three keyframe selections (rgc_uniform_sampling, rgc_kf_get_travel,
rgc_kf_select_surrounding / _global, rgc_kf_detect_loop).  numpy only; the leaf grid is pre_reference's (imported, not modified), everything else is
written from the definitions in include/rgc_hip.h and src/RGC_mapping.cpp:1525-1548, 1887-1908, 2141-2225, 2493-2505.  Every operation is a single
correctly rounded fp32 operation, so the results are exact by construction:

    centre of a leaf   c_a = fp32(fp32(fp32(ijk_a) + 0.5f) * leaf),  ijk = floor(fp32(p * inv)) (the GLOBAL leaf coordinate)
    key of a point     d2 = fp32(fp32(fp32(dx*dx) + fp32(dy*dy)) + fp32(dz*dz))
    winner of a leaf   the member with the smallest (d2, input index); leaves in ascending leaf index
    radius gate        r2 = fp32(fp64(radius) * fp64(radius)); inside when d2 < r2 (strict)."""
import numpy as np

import pre_reference as pr

F = np.float32


def dist2(p, q):
    """(dx*dx + dy*dy) + dz*dz in fp32, one rounding per operation; p (n, 3), q (3,) or (n, 3)"""
    d = np.asarray(p, F) - np.asarray(q, F)
    assert d.dtype == F
    dd = d * d
    out = (dd[..., 0] + dd[..., 1]) + dd[..., 2]
    assert out.dtype == F
    return out


def leaf_centres(xyz, leaf):
    ijk = pr.leaf_coords(xyz, leaf)
    c = (ijk.astype(F) + F(0.5)) * F(leaf)
    assert c.dtype == F
    return c


class UniformSamplingResult:
    """out (m, 4) float32: the winners' points; index (m,) int64: their input indices; first (m,) int64: each leaf's first member; ties (m,) bool: more
    than one member holds the leaf's minimum key; leaf: the LeafFilterResult the leaves come from (unfiltered: out is the input, index the identity)"""

    def __init__(self, out, index, first, ties, leaf):
        self.out, self.index, self.first, self.ties, self.leaf = out, index, first, ties, leaf

    @property
    def unfiltered(self):
        return self.leaf.unfiltered

    def census(self):
        return dict(leaves=len(self.index), tie_leaves=int(self.ties.sum()), winner_not_first=int((self.index != self.first).sum()),
                    fullest=self.leaf.fullest)


def uniform_sampling(xyzc, leaf, by_members=False):
    p = pr.four_columns(xyzc)
    n = p.shape[0]
    r = pr.voxelgrid(p, leaf)
    if r.unfiltered:
        i = np.arange(n, dtype=np.int64)
        return UniformSamplingResult(p.copy(), i, i, np.zeros(n, bool), r)
    m = len(r.out)
    if n == 0:
        z = np.zeros(0, np.int64)
        return UniformSamplingResult(p.copy(), z, z, np.zeros(0, bool), r)
    key = dist2(p[:, :3], leaf_centres(p[:, :3], leaf))
    if by_members:                               # leaf by leaf, through LeafFilterResult.members: the definition
        index, first, ties = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, bool)
        for j in range(m):
            mem = r.members(j)                   # ascending input index
            k = key[mem]
            w = int(np.argmin(k))                # the FIRST minimum: the smallest (d2, index)
            index[j], first[j], ties[j] = mem[w], mem[0], int((k == k[w]).sum()) > 1
    else:                                        # the same over all leaves at once: members(j) = order[start[j]:start[j + 1]]
        ko = key[r.order]
        leaf_of = np.repeat(np.arange(m), np.diff(r.start))
        slots = np.flatnonzero(ko == np.minimum.reduceat(ko, r.start[:-1])[leaf_of])        # every slot that holds its leaf's minimum, ascending
        _, firsts, counts = np.unique(leaf_of[slots], return_index=True, return_counts=True)
        index, first, ties = r.order[slots[firsts]], r.order[r.start[:-1]], counts > 1
    return UniformSamplingResult(p[index].copy(), index, first, ties, r)


# ---- the store's travelled distance and angle (:1887-1908) ----------------------------------------------------------------------------
def travel_step(prev_distance, prev_angle, prev_pose, pose):
    """one push: (distance, angle) fp32 from the previous keyframe's values and the pose stored for it at that moment; poses = (x, y, z, roll, pitch, yaw)"""
    a, b = np.asarray(pose, F), np.asarray(prev_pose, F)
    d = a[:3] - b[:3]
    dd = d * d
    dis = F(prev_distance) + np.sqrt((dd[0] + dd[1]) + dd[2])
    rad = F(a[5] - b[5])
    if np.float64(rad) > np.pi:
        rad = F(np.float64(rad) - np.pi * 2)
    if np.float64(rad) < -np.pi:
        rad = F(np.float64(rad) + np.pi * 2)
    ang = F(prev_angle) + np.abs(rad)
    assert dis.dtype == F and ang.dtype == F
    return dis, ang


def travel(poses):
    """a drive pushed pose by pose with no correction in between: (distance (n,), angle (n,)) fp32, vectorised (a sequential fp32 running sum)"""
    p = np.asarray(poses, F).reshape(-1, 6)
    n = len(p)
    if n == 0:
        return np.zeros(0, F), np.zeros(0, F)
    step = np.sqrt(dist2(p[1:, :3], p[:-1, :3]))
    rad = p[1:, 5] - p[:-1, 5]
    r64 = rad.astype(np.float64)
    rad = np.where(r64 > np.pi, (r64 - np.pi * 2).astype(F), rad)
    r64 = rad.astype(np.float64)
    rad = np.where(r64 < -np.pi, (r64 + np.pi * 2).astype(F), rad).astype(F)
    dis = np.add.accumulate(np.concatenate([[F(0)], step]).astype(F), dtype=F)
    ang = np.add.accumulate(np.concatenate([[F(0)], np.abs(rad)]).astype(F), dtype=F)
    return dis, ang


# ---- the selections -------------------------------------------------------------------------------------------------------------------
def gate(xyz, query, radius):
    """(inside (n,) bool, d2 (n,) fp32, r2)"""
    r2 = F(np.float64(F(radius)) * np.float64(F(radius)))
    d2 = dist2(np.asarray(xyz, F).reshape(-1, 3), np.asarray(query, F))
    return d2 < r2, d2, r2


def select_surrounding(xyz, ids, center, radius, density):
    """-> (ids of the winners in ascending leaf index, number inside the radius, the UniformSamplingResult or None)"""
    xyz, ids = np.asarray(xyz, F).reshape(-1, 3), np.asarray(ids)
    inside, _, _ = gate(xyz, center, radius)
    pos = np.flatnonzero(inside)                   # ascending store position
    if len(pos) == 0:
        return ids[:0].copy(), 0, None
    us = uniform_sampling(xyz[pos], density)
    return ids[pos[us.index]], len(pos), us


def select_global(xyz, ids, density):
    xyz, ids = np.asarray(xyz, F).reshape(-1, 3), np.asarray(ids)
    if len(xyz) == 0:
        return ids[:0].copy(), None
    us = uniform_sampling(xyz, density)
    return ids[us.index], us


LOOP_DEFAULTS = dict(history_search_radius=5.0, drift_factor=0.02, distance_by_loop=0.0, loop_keyframe_dis_diff=20.0, history_search_num=50, min_key_id=10)


def _loop_setup(xyz, travel_d, prm):
    L = len(xyz) - 1
    R = F(prm["history_search_radius"]) + (F(travel_d[L]) - F(prm["distance_by_loop"])) * F(prm["drift_factor"])
    thr = F(prm["loop_keyframe_dis_diff"]) + R
    assert R.dtype == F and thr.dtype == F
    inside, d2, _ = gate(xyz, xyz[L], R)
    passes = np.abs(np.asarray(travel_d, F) - F(travel_d[L])) > thr
    return L, R, inside, d2, passes


def _loop_finish(L, R, inside, pc, ids, n_feature, prm, skipped):
    out = dict(found=False, latest_id=int(ids[L]), closest_id=-1, closest_pos=-1, search_radius=R, n_in_radius=int(inside.sum()), history_ids=[],
               nearer_skipped_for_id=skipped)
    if pc < 0:
        return out
    out["closest_id"], out["closest_pos"] = int(ids[pc]), int(pc)
    if ids[pc] == ids[L]:
        return out
    pts = 0
    for i in range(-int(prm["history_search_num"]), int(prm["history_search_num"]) + 1):
        p = pc + i
        if p < 0 or p >= L:
            continue
        if ids[p] < 0 or ids[p] >= ids[L]:
            continue
        out["history_ids"].append(int(ids[p]))
        pts += int(n_feature[p])
    out["found"] = pts > 0
    return out


def detect_loop(xyz, ids, travel_d, n_feature, **params):
    """the arg-min form: the qualifying pose with the smallest (d2, position).  n_feature[p] = corner + surf points of position p."""
    prm = dict(LOOP_DEFAULTS, **params)
    xyz, ids = np.asarray(xyz, F).reshape(-1, 3), np.asarray(ids)
    if len(xyz) == 0:
        return dict(found=False, latest_id=-1, closest_id=-1, closest_pos=-1, search_radius=F(0), n_in_radius=0, history_ids=[], nearer_skipped_for_id=0)
    L, R, inside, d2, passes = _loop_setup(xyz, travel_d, prm)
    q = np.flatnonzero(inside & passes & (ids >= prm["min_key_id"]))
    pc = -1
    skipped = 0
    if len(q):
        pc = int(q[np.lexsort((q, d2[q]))[0]])
        low = np.flatnonzero(inside & passes & (ids < prm["min_key_id"]))
        skipped = int(((d2[low] < d2[pc]) | ((d2[low] == d2[pc]) & (low < pc))).sum())
    return _loop_finish(L, R, inside, pc, ids, n_feature, prm, skipped)


def detect_loop_literal(xyz, ids, travel_d, n_feature, **params):
    """the reference's text, :2157-2172: the radius result sorted by (d2, position), walked; `continue` on id < min, `break` at the first that passes"""
    prm = dict(LOOP_DEFAULTS, **params)
    xyz, ids = np.asarray(xyz, F).reshape(-1, 3), np.asarray(ids)
    if len(xyz) == 0:
        return detect_loop(xyz, ids, travel_d, n_feature, **params)
    L, R, inside, d2, passes = _loop_setup(xyz, travel_d, prm)
    found_idx = np.flatnonzero(inside)
    found_idx = found_idx[np.lexsort((found_idx, d2[found_idx]))]
    pc, skipped = -1, 0
    for index in found_idx:
        key_id = ids[index]
        if passes[index]:
            if key_id < prm["min_key_id"]:
                skipped += 1
                continue
            pc = int(index)
            break
    if pc < 0:
        skipped = 0
    return _loop_finish(L, R, inside, pc, ids, n_feature, prm, skipped)
