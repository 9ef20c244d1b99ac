"""An independent reference for the FPFH descriptors (rgc_fpfh_estimate): numpy and scipy only, written from the text of include/rgc_hip.h, nothing from
oracle/ and nothing from the product.

Rows: those the search reference stands on (tests/gicp_mp_reference.radius_rows, which tests/search_reference.radius_csr sorts: fp64 cKDTree candidates with
a margin, the fp32 key ((dx dx + dy dy) + dz dz) recomputed with float32 ufuncs, every row PROVEN complete) -- every surface point with key < float32(r r),
strict.  Nothing here depends on the order inside a row.

Pair terms: in numpy longdouble from the float32 inputs, exactly as the header orders them (d = t - s, f4, c1, c2, the swap on the numerators, v = d x u, vn,
w = u x v, f2, f1 = atan2, f3, the three bin coordinates x = 11 ((f1 + pi) / (2 pi)), 11 ((f2 + 1) / 2), 11 ((f3 + 1) / 2), floor, clamp to 0 .. 10).  A pair
is UNDECIDED -- an fp64 evaluation may land in another bin, swap differently or skip differently -- when
  * a bin coordinate lies within 1e-9 max(1, f4 / vn) of an interior wall (the integers 1 .. 10): an fp64 pair term carries some tens of 2^-53 relative, v / vn
    amplifies the rounding of the cross product by f4 |u| / vn, and 1e-9 leaves six decimal orders above that;
  * 0 < ||c1| - |c2|| < 1e-12 (|c1| + |c2|): the swap could go either way;
  * 0 < vn < 1e-12 f4 |u|: an fp64 cross product could cancel to exactly 0 where this one does not.
Exact ties (|c1| == |c2|) and an exact vn == 0 are DECIDED: on dyadic coordinates and axis-aligned normals both are bit-exact in any arithmetic.

SPFH: integer counts per surface point of its non-skipped pairs, m_s = the row size (skipped pairs included), und[s] = its undecided pairs.

FPFH: F[b] = sum over the row members j with key > 0, j valid (and m_j > 1) of (count_j[b] * (100 / (m_j - 1))) * (1 / key_j), in longdouble; per block of 11
out[b] = F[b] * (100 / sum) when sum != 0, else 0.  bound[q, b]: every term is non-negative, so the error of ANY fp64 evaluation is relative.  With u = 2^-53
and t = the number of contributing members of q: a term is three roundings (inc, the product with the count, the product with w) on top of w's own, (1 + u)^4;
a t-term sum in any order adds (1 + u)^(t - 1); the block's sum of 11 such entries (1 + u)^10 more; 100 / sum and the last product one each: the quotient
F[b] * (100 / sum) errs by at most ((t + 3) + (t + 13) + 2) u = (2 t + 18) u relative, taken as (2 t + 24) u for the second-order terms and this reference's own
2^-64 roundings.  The fp32 store adds at most one fp32 ulp of the entry:
  bound = |out| (2 t + 24) 2^-53 + spacing(float32(|out|)).
tainted[q]: some member of q owns an undecided pair -- its counts may differ, the bound does not apply."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import gicp_mp_reference as mr

LD = np.longdouble
U = 2.0 ** -53
BINS = 33
WALL_EPS, SWAP_EPS, VN_EPS = 1e-9, 1e-12, 1e-12
CHUNK = 1 << 16


def _xyz(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)[:, :3])


def _chunks(f, starts):
    """f(start) of every chunk, in order; numpy's loops release the interpreter, so a few threads share the longdouble arithmetic of a long case"""
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        yield from pool.map(f, starts)


def pair_terms(S, A, T, B):
    """the pair terms of surface points S (m, 3) with normals A against members T with normals B (all longdouble, both valid, key > 0): dict of the
    bins (m, 3) int64, skipped (vn == 0), swapped, tie (|c1| == |c2| exactly), undecided"""
    d = T - S
    f4 = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    c1 = (A[:, 0] * d[:, 0] + A[:, 1] * d[:, 1]) + A[:, 2] * d[:, 2]
    c2 = (B[:, 0] * d[:, 0] + B[:, 1] * d[:, 1]) + B[:, 2] * d[:, 2]
    swap = np.abs(c1) < np.abs(c2)
    tie = np.abs(c1) == np.abs(c2)
    sw = swap[:, None]
    u, n2 = np.where(sw, B, A), np.where(sw, A, B)
    d = np.where(sw, -d, d)
    with np.errstate(invalid="ignore", divide="ignore"):
        f3 = np.where(swap, -c2, c1) / f4
        v = np.stack([d[:, 1] * u[:, 2] - d[:, 2] * u[:, 1], d[:, 2] * u[:, 0] - d[:, 0] * u[:, 2], d[:, 0] * u[:, 1] - d[:, 1] * u[:, 0]], axis=1)
        vn = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        skipped = vn == 0
        v = v / vn[:, None]
        w = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
        f2 = (v[:, 0] * n2[:, 0] + v[:, 1] * n2[:, 1]) + v[:, 2] * n2[:, 2]
        f1 = np.arctan2((w[:, 0] * n2[:, 0] + w[:, 1] * n2[:, 1]) + w[:, 2] * n2[:, 2], (u[:, 0] * n2[:, 0] + u[:, 1] * n2[:, 1]) + u[:, 2] * n2[:, 2])
        pi = LD("3.14159265358979323846264338327950288")
        x = np.stack([LD(11) * ((f1 + pi) * (LD(1) / (LD(2) * pi))), LD(11) * ((f2 + LD(1)) * LD(0.5)), LD(11) * ((f3 + LD(1)) * LD(0.5))], axis=1)
        xs = np.where(skipped[:, None], LD(0.5), x)
        bins = np.clip(np.floor(xs), 0, 10).astype(np.int64)
        un = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
        amp = np.maximum(LD(1), np.where(skipped, LD(1), f4 / vn))
        near = (np.abs(xs - np.rint(xs)) < WALL_EPS * amp[:, None]) & (np.rint(xs) >= 1) & (np.rint(xs) <= 10)
        gap = np.abs(np.abs(c1) - np.abs(c2))
        und = (near.any(axis=1) & ~skipped) | ((gap > 0) & (gap < SWAP_EPS * (np.abs(c1) + np.abs(c2)))) | ((vn > 0) & (vn < VN_EPS * f4 * un))
    return dict(bins=bins, skipped=skipped, swapped=swap, tie=tie, undecided=und)


def spfh(surface, normals, radius, rows=None):
    """the first pass over EVERY surface point: counts (ns, 33) int64, m (ns,), valid (ns,), und (ns,) undecided pairs owned, and the census of the pairs;
    rows: radius_rows(surface, surface, radius) where the caller has them"""
    T = _xyz(surface)
    N = np.asarray(normals, np.float32)[:, :3]
    ns = len(T)
    valid = np.isfinite(N).all(axis=1)
    rows = rows or mr.radius_rows(T, T, radius)
    off, row, idx, key = rows["off"], rows["row"], rows["idx"], rows["key"]
    m = np.diff(off)
    counts = np.zeros((ns, BINS), np.int64)
    und = np.zeros(ns, np.int64)
    census = dict(members=int(len(idx)), key0=int((key == 0).sum()) - ns, invalid_members=int((valid[row] & ~valid[idx] & (key > 0)).sum()), pairs=0, computed=0, swaps=0, ties=0,
                  vn0=0, undecided=0)
    use = np.flatnonzero(valid[row] & valid[idx] & (key > 0))
    census["pairs"] = int(len(use))
    Tl, Nl = T.astype(LD), np.where(valid[:, None], N, 0).astype(LD)

    def chunk(a):
        sel = use[a:a + CHUNK]
        s, t = row[sel], idx[sel]
        return s, pair_terms(Tl[s], Nl[s], Tl[t], Nl[t])

    for s, p in _chunks(chunk, range(0, len(use), CHUNK)):
        ok = ~p["skipped"]
        for blk in range(3):
            counts += np.bincount(s[ok] * BINS + blk * 11 + p["bins"][ok, blk], minlength=ns * BINS).reshape(ns, BINS)
        und += np.bincount(s[p["undecided"]], minlength=ns)
        census["computed"] += int(ok.sum())
        census["swaps"] += int(p["swapped"].sum())
        census["ties"] += int(p["tie"].sum())
        census["vn0"] += int(p["skipped"].sum())
        census["undecided"] += int(p["undecided"].sum())
    census["skipped"] = census["members"] - ns - census["computed"]      # key 0 beyond the point itself, an invalid end, vn == 0
    census["owners"] = int((und > 0).sum())
    return dict(counts=counts, m=m.astype(np.int32), valid=valid, und=und, census=census)


def estimate(queries, normals, radius, surface=None) -> dict:
    """everything the device is compared with (see the module docstring)"""
    Q = _xyz(queries)
    T = Q if surface is None else _xyz(surface)
    nq, ns = len(Q), len(T)
    rows = mr.radius_rows(T, Q, radius)
    first = spfh(T, normals, radius, rows if surface is None else None)
    counts, m_s, valid, und = first["counts"], first["m"], first["valid"], first["und"]
    off, row, idx, key = rows["off"], rows["row"], rows["idx"], rows["key"]
    m_q = np.diff(off)
    computed = np.ones(ns, bool)
    if surface is not None:
        computed = np.zeros(ns, bool)
        computed[idx] = True
    use = np.flatnonzero((key > 0) & valid[idx] & (m_s[idx] > 1))
    with np.errstate(divide="ignore"):
        A = counts.astype(LD) * (LD(100) / np.maximum(m_s - 1, 1).astype(LD))[:, None]      # SPFH as numbers: count * inc
    F = np.zeros((nq, BINS), LD)

    def chunk(a):                                           # (the members of a row are consecutive: segment sums; a row cut by a chunk is added to twice)
        sel = use[a:a + CHUNK // 4]
        w = LD(1) / key[sel].astype(LD)
        cut = np.flatnonzero(np.diff(row[sel], prepend=-1))
        return row[sel][cut], np.add.reduceat(A[idx[sel]] * w[:, None], cut, axis=0)

    for r, part in _chunks(chunk, range(0, len(use), CHUNK // 4)):
        F[r] += part
    terms = np.bincount(row[use], minlength=nq)
    tainted = np.bincount(row[use], weights=(und[idx[use]] > 0), minlength=nq) > 0
    out = np.zeros((nq, BINS), LD)
    for blk in range(3):
        b = slice(blk * 11, blk * 11 + 11)
        s = F[:, b].sum(axis=1)
        nz = s != 0
        out[nz, b] = F[nz, b] * (LD(100) / s[nz])[:, None]
    out = out.astype(np.float64)
    out[m_q == 0] = np.nan
    with np.errstate(invalid="ignore"):
        bound = np.abs(out) * ((2.0 * terms + 24.0) * U)[:, None] + np.spacing(np.abs(out).astype(np.float32)).astype(np.float64)
    return dict(fpfh=out, bound=bound, count=m_q.astype(np.int32), n_valid=int((m_q > 0).sum()), tainted=tainted, terms=terms, spfh=counts, spfh_und=und,
                spfh_count=np.where(computed, m_s, -1).astype(np.int32), computed=computed, n_spfh=int(computed.sum()), valid=valid, census=first["census"],
                empty_rows=int((m_q == 0).sum()), max_count=int(counts.max()) if counts.size else 0, max_members=int(m_q.max()) if nq else 0)
