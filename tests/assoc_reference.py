"""An independent reference for the mapping node's feature association (numpy / scipy only; nothing from oracle/).

Per feature: pointAssociateToMap (q * p + t in fp64, stored as float32); the 5 nearest map points by (fp32 key, original index) through
``nn_reference``; the gate ``key[4] < 1.0`` (edge) / ``< 2.0`` (plane), compared in fp32, exactly; then
  edge   centred 3x3 scatter of the five, ``np.linalg.eigh``, kept when ``l1 > 3 l2``; the factor is ``centre +- 0.1 v1``
  plane  ``np.linalg.lstsq`` of ``A n = -1``, normalised; kept when every ``|n.p + d| <= 0.2``.
Every feature also gets a MARGIN: how far its decision is from flipping -- ``|l1 - 3 l2| / l1`` (edge), the smallest
``||n.p + d| - 0.2|`` over the five (plane).  A feature is DECIDED when its margin exceeds ``MARGIN_MIN = 1e-9``: six orders above fp64
rounding on these 5-point problems, far below anything geometry produces by chance.  A plane fit whose 5x3 matrix is rank-deficient to
fp64 (five collinear points, or five coplanar with the origin) is undecided too: a column-pivoted QR returns a basic solution there,
``lstsq`` the minimum-norm one, and neither is "the" answer.  Features the gate rejects are decided (the gate is exact).
"""
from __future__ import annotations

import numpy as np

import nn_reference as nnr

MARGIN_MIN = 1e-9
UNDECIDED_MAX = 0.005      # at most this fraction of a case may be undecided


def associate_to_map(feat, q_xyzw, t) -> np.ndarray:
    """Eigen's quaternion * vector (v + w * 2(u x v) + u x 2(u x v)) plus t, fp64, stored as float32"""
    p = np.asarray(feat, np.float32)[:, :3].astype(np.float64)
    x, y, z, w = (float(v) for v in q_xyzw)
    u = np.array([x, y, z])
    uv = 2.0 * np.cross(u, p)
    out = p + w * uv + np.cross(u, uv) + np.asarray(t, np.float64)
    return out.astype(np.float32)


def associate(feat, q_xyzw, t, map_xyz, kind: str) -> dict:
    """dict(valid, decided, margin, gate (passed the 5th-neighbour gate), idx (n,5), key (n,5), var, and a, b (edge) or n, d (plane))"""
    assert kind in ("edge", "plane")
    feat = np.asarray(feat, np.float32)
    M = np.ascontiguousarray(np.asarray(map_xyz, np.float32)[:, :3])
    nf = feat.shape[0]
    S = associate_to_map(feat, q_xyzw, t)
    valid = np.zeros(nf, bool)
    decided = np.ones(nf, bool)
    margin = np.full(nf, np.inf)
    out = dict(valid=valid, decided=decided, margin=margin, var=np.zeros(nf), moved=S)
    if kind == "edge":
        out.update(a=np.zeros((nf, 3)), b=np.zeros((nf, 3)))
    else:
        out.update(n=np.zeros((nf, 3)), d=np.zeros(nf))
    if M.shape[0] < 5:
        out.update(gate=np.zeros(nf, bool), idx=np.full((nf, 5), -1), key=np.full((nf, 5), np.inf, np.float32))
        return out
    idx, key = nnr.nearest_k(M, S, 5)
    limit = np.float32(1.0 if kind == "edge" else 2.0)
    gate = key[:, 4] < limit                                  # float32 < float32
    out.update(gate=gate, idx=idx, key=key)
    M64 = M.astype(np.float64)
    for i in np.nonzero(gate)[0]:
        Q = M64[idx[i]]
        if kind == "edge":
            c = Q.mean(0)
            Z = Q - c
            w, V = np.linalg.eigh(Z.T @ Z)                    # ascending
            l1, l2 = w[2], w[1]
            margin[i] = abs(l1 - 3.0 * l2) / l1 if l1 > 0 else 0.0
            if l1 > 3.0 * l2:
                valid[i] = True
                out["a"][i], out["b"][i] = c + 0.1 * V[:, 2], c - 0.1 * V[:, 2]
        else:
            if np.linalg.matrix_rank(Q) < 3:
                decided[i] = False
                margin[i] = 0.0
                continue
            n, *_ = np.linalg.lstsq(Q, -np.ones(5), rcond=None)
            nn = np.linalg.norm(n)
            d = 1.0 / nn
            n = n / nn
            r = np.abs(Q @ n + d)
            margin[i] = np.abs(r - 0.2).min()
            if (r <= 0.2).all():
                valid[i] = True
                out["n"][i], out["d"][i] = n, d
        if margin[i] <= MARGIN_MIN:
            decided[i] = False
    out["var"] = np.where(valid, feat[:, 3].astype(np.float64), 0.0)
    return out


def compare(got: dict, ref: dict, kind: str, tol=1e-9, mid_tol=1e-12) -> dict:
    """The decided-feature rule.  got: a dict with valid / a, b / n, d / var (the product's or the oracle's); ref: associate()'s.
    Asserts: at most UNDECIDED_MAX of the features undecided, flags equal on every decided feature, factors to tol (an edge's two points
    up to the free sign of the eigenvector, their mid-point to mid_tol), var equal.  Returns the figures it looked at."""
    dec = ref["decided"]
    n = len(dec)
    n_und = int((~dec).sum())
    assert n_und <= UNDECIDED_MAX * n, f"{n_und} of {n} features undecided: the case sits on thresholds"
    gv, rv = np.asarray(got["valid"], bool), ref["valid"]
    bad = np.nonzero(dec & (gv != rv))[0]
    assert bad.size == 0, f"valid flags differ on {bad.size} decided features, first {bad[:8].tolist()} (margins {ref['margin'][bad[:8]].tolist()})"
    both = dec & gv & rv
    fig = dict(n=n, undecided=n_und, valid=int(rv.sum()), compared=int(both.sum()), err=0.0, mid_err=0.0)
    if both.any():
        if kind == "edge":
            d1 = np.maximum(np.abs(got["a"][both] - ref["a"][both]).max(axis=1), np.abs(got["b"][both] - ref["b"][both]).max(axis=1))
            d2 = np.maximum(np.abs(got["a"][both] - ref["b"][both]).max(axis=1), np.abs(got["b"][both] - ref["a"][both]).max(axis=1))
            fig["err"] = float(np.minimum(d1, d2).max())
            fig["mid_err"] = float(np.abs(0.5 * (got["a"][both] + got["b"][both]) - 0.5 * (ref["a"][both] + ref["b"][both])).max())
            assert fig["mid_err"] < mid_tol, f"edge mid-points differ by {fig['mid_err']:.3e}"
        else:
            fig["err"] = float(max(np.abs(got["n"][both] - ref["n"][both]).max(), np.abs(np.asarray(got["d"])[both] - ref["d"][both]).max()))
        assert fig["err"] < tol, f"{kind} factors differ by {fig['err']:.3e}"
        assert np.array_equal(np.asarray(got["var"])[both], ref["var"][both])
    return fig
