"""An independent reference for the outlier filters (rgc_outlier_statistical / rgc_outlier_radius): numpy and scipy only, nothing from oracle/ and
nothing from the product.

Rows come from search_reference.knn_rows / radius_csr, which are PROVEN complete under the product's fp32 key ((dx dx + dy dy) + dz dz).  On top:

* d_i = float32(sum over ranks 1 .. mean_k of float64(sqrt_f32(key_r)) / mean_k): a sequential fp64 loop over the ranks, so bit-exact by construction
  (rank 0, the point itself or a duplicate of it, is dropped; tied keys have equal roots, so the order among ties is immaterial).  sqrt_f32 is numpy's
  float32 square root, which is correctly rounded.
* sum = fsum(d), sq_sum = fsum(float64(d)^2) (math.fsum: correctly rounded; the squares are exact in fp64), then mean / variance (clamped at 0) / stddev /
  threshold in longdouble.
* threshold_bound(): how far a threshold computed in fp64 with ANY order of the two sums may lie from that reference.  Derived, not chosen:

      u = 2^-53.  Summing n non-negative doubles in any order gives S^ = S (1 + e), |e| <= g = (n - 1) u / (1 - (n - 1) u)   (Higham, Accuracy and
      Stability, eq. 4.4 with all terms of one sign).  Every further fp64 operation adds one relative rounding of at most u.
      mean^ = fl(S^ / n)                                  |mean^ - mean| <= (g + u (1 + g)) mean                       =: E_mean
      A = S S / n, two roundings on top of (1 + e)^2:     |A^ - A| <= ((1 + g)^2 (1 + u)^2 - 1) A                      =: E_A
      N = Q - A, one rounding of the difference:          |N^ - N| <= g Q + E_A + u (|N| + g Q + E_A)                  =: E_N
      V = max(N / (n - 1), 0), one rounding (the clamp moves V^ no farther from a V >= 0):
                                                          |V^ - V| <= E_N / (n - 1) + u (V + E_N / (n - 1))            =: E_V
      s = sqrt(V), correctly rounded: |sqrt(a) - sqrt(b)| <= min(sqrt|a - b|, |a - b| / sqrt(b)), so
                                                          |s^ - s| <= min(sqrt(E_V), E_V / s) + u (s + min(..))        =: E_s
      t = mean + m s, a product and a sum:                |t^ - t| <= E_mean + |m| E_s + u |m| (s + E_s) + u (|t| + E_mean + |m| (E_s + u (s + E_s)))

  statistics() is itself a computation of this form -- math.fsum rounds each exact sum once (g = u), longdouble operations round at 2^-64 -- so its own
  distance from the exact value, the same chain with g = u and 2^-63 for u, is added: the bound holds between the device and THIS reference.
  Exact case: when every d_i is the same float d and n is a power of two not above 32, every partial sum of either column is (an integer <= 32) x (d or
  d d), which fits 53 bits (24 + 5, 48 + 5): both sums are exact in any order, S / n = d, S S / n = n d d = Q, V = 0 and t = d exactly: the bound is 0.
  (n = 2 with mean_k = 1 is always this case: the two points are each other's only neighbour at the same key.)

A point is UNDECIDED when |d_i - threshold| <= bound with bound > 0: the device may then decide it either way.  The designed cases keep that number at 0."""
from __future__ import annotations

import math

import numpy as np

import search_reference as sr

U = 2.0 ** -53


def mean_distances(cloud, mean_k: int) -> np.ndarray:
    """(n,) float32"""
    P = sr._xyz(cloud)
    assert len(P) > mean_k >= 1
    _, key = sr.knn_rows(P, P, mean_k + 1)
    root = np.sqrt(key.astype(np.float32)).astype(np.float64)          # float32 sqrt (correctly rounded), widened
    s = np.zeros(len(P), np.float64)
    for r in range(1, mean_k + 1):                                     # sequential fp64 sum in ascending rank
        s = s + root[:, r]
    return (s / np.float64(mean_k)).astype(np.float32)


def statistics(d, std_mul: float) -> dict:
    """mean, stddev, threshold (longdouble) and the two correctly rounded sums of the float32 mean distances d"""
    d64 = np.asarray(d, np.float32).astype(np.float64)
    n = len(d64)
    S, Q = math.fsum(d64), math.fsum(d64 * d64)
    L = np.longdouble
    mean = L(S) / L(n)
    var = (L(Q) - L(S) * L(S) / L(n)) / L(n - 1)
    var = max(var, L(0))
    std = np.sqrt(var)
    return dict(n=n, sum=S, sq_sum=Q, mean=mean, stddev=std, threshold=mean + L(std_mul) * std)


def _propagate(n, S, Q, mean, s, t, m, g, u):
    """the chain of the module docstring for sums of relative error g and operations of relative rounding u (all longdouble)"""
    e_mean = (g + u * (1 + g)) * mean
    A = S * S / n
    e_a = ((1 + g) ** 2 * (1 + u) ** 2 - 1) * A
    e_n = g * Q + e_a + u * (abs(Q - A) + g * Q + e_a)
    e_v = e_n / (n - 1) + u * (s * s + e_n / (n - 1))
    e_root = np.sqrt(e_v) if s == 0 else min(np.sqrt(e_v), e_v / s)
    e_s = e_root + u * (s + e_root)
    e_prod = m * e_s + u * m * (s + e_s)
    return e_mean + e_prod + u * (t + e_mean + e_prod)


def threshold_bound(d, std_mul: float) -> float:
    """the bound of the module docstring on |threshold (fp64, any summation order) - statistics()['threshold']|"""
    d64 = np.asarray(d, np.float32).astype(np.float64)
    n = len(d64)
    if n <= 32 and n & (n - 1) == 0 and (d64 == d64[0]).all():
        return 0.0
    st = statistics(d, std_mul)
    L = np.longdouble
    S, Q, m, u = L(st["sum"]), L(st["sq_sum"]), abs(L(std_mul)), L(U)
    args = (n, S, Q, st["mean"], st["stddev"], abs(st["threshold"]), m)
    device = _propagate(*args, g=(n - 1) * u / (1 - (n - 1) * u), u=u)
    reference = _propagate(*args, g=u, u=L(2.0) ** -63)          # statistics() itself: fsum rounds each sum once, longdouble rounds at 2^-64 (2^-63 taken)
    return float(device + reference)


def sor(cloud, mean_k: int, std_mul: float) -> dict:
    """everything the SOR tests compare with: d, the statistics, the bound, the inlier mask (d <= threshold) and the undecided points"""
    d = mean_distances(cloud, mean_k)
    st = statistics(d, std_mul)
    b = threshold_bound(d, std_mul)
    gap = np.abs(d.astype(np.longdouble) - st["threshold"])
    return dict(d=d, bound=b, inlier=d.astype(np.longdouble) <= st["threshold"], undecided=int(((gap <= b) & (b > 0)).sum()), min_gap=float(gap.min()), **st)


def counts(cloud, radius: float) -> np.ndarray:
    """(n,) int32: the cloud's points with key < float32(radius^2) about every point, itself included"""
    P = sr._xyz(cloud)
    off, _, _ = sr.radius_csr(P, P, radius, 0)
    return np.diff(off).astype(np.int32)


def ror_inlier(count, min_neighbors: int) -> np.ndarray:
    return np.asarray(count) - 1 >= int(min_neighbors)


# ---- brute force: every pair's fp32 key (search_reference.all_keys); pins the wrappers above on small clouds ----
def brute_mean_distances(cloud, mean_k: int) -> np.ndarray:
    K = np.sort(sr.all_keys(cloud, cloud), axis=1)[:, 1:mean_k + 1]
    root = np.sqrt(K.astype(np.float32)).astype(np.float64)
    s = np.zeros(len(K), np.float64)
    for r in range(mean_k):
        s = s + root[:, r]
    return (s / np.float64(mean_k)).astype(np.float32)


def brute_counts(cloud, radius: float) -> np.ndarray:
    import gicp_mp_reference as mr
    return (sr.all_keys(cloud, cloud) < mr.r2_of(radius)).sum(axis=1).astype(np.int32)
