"""The grid walks' census: the integer read-outs that the walk ALONE determines (`candidates`, `grown`, rgc_gicpmp_num_candidates) and a SHA-256 of
FastGICPMultiPoints' merged() bytes (the order of those fp64 sums is the walk's), for every designed case of search_cases, outlier_cases, cluster_cases
and gicp_mp_cases at the cell sizes their GPU tests use.  census() runs the product only; tests/golden/gen_walk_census.py records it into
tests/golden/fx_walk_census.json and tests/test_gpu_walk_census.py holds the library equal to the record.

Keys:  search/<case>/cell=<c>/knn/k=<k>         one k per list tier (4, 8, 16, 32): the largest of the case's ks in the tier
       search/<case>/cell=<c>/radius/r=<r>/max_nn=<m>   the cells of test_radius_rows_equal_the_reference (automatic and the case's first)
       outlier/<case>/cell=<c>/sor/mean_k=<k>    outlier/<case>/cell=<c>/ror/r=<r>/min=<m>/exact|early
       cluster/<case>/tol=<t>/cell=<c>           (the limits do not reach the walk: the case's first pair)
       gicp_mp/<case>/pose=<p>                   candidates and the digest of merged()"""
import hashlib

import numpy as np

import cluster_cases as cc
import gicp_mp_cases as mc
import outlier_cases as oc
import search_cases as sc

TIERS = (4, 8, 16, 32)


def tier_ks(ks):
    """the largest k of ks in every list tier that ks reaches"""
    out, lo = [], 0
    for t in TIERS:
        inside = [k for k in ks if lo < k <= t]
        if inside:
            out.append(max(inside))
        lo = t
    return out


def search_census(out):
    from rgc_slam_amd import search
    tree = search.KdTree(0)
    try:
        for case in sc.all_cases():
            for cell in (0.0,) + tuple(case["cells"]):
                tree.setInputCloud(case["tgt"], cell)
                base = "search/%s/cell=%g" % (case["name"], cell)
                for k in tier_ks(case["ks"]):
                    tree.nearestKSearch(case["qry"], k)
                    info = tree.info()
                    out["%s/knn/k=%d" % (base, k)] = dict(candidates=int(info["candidates"]), grown=int(info["grown"]))
                if cell in (0.0,) + tuple(case["cells"][:1]):
                    for r, max_nn in case["radii"]:
                        tree.radiusSearch(case["qry"], r, max_nn, True)
                        info = tree.info()
                        out["%s/radius/r=%r/max_nn=%d" % (base, r, max_nn)] = dict(candidates=int(info["candidates"]), grown=int(info["grown"]))
    finally:
        tree.close()


def outlier_census(out):
    from rgc_slam_amd import filters
    sor, ror = filters.StatisticalOutlierRemoval(0), filters.RadiusOutlierRemoval(0)
    try:
        for case in oc.all_cases():
            for cell in (0.0,) + tuple(case["cells"]):
                sor.setCell(cell)
                ror.setCell(cell)
                base = "outlier/%s/cell=%g" % (case["name"], cell)
                for mean_k, std_mul in case["sor"]:
                    sor.setInputCloud(case["cloud"])
                    sor.setMeanK(mean_k)
                    sor.setStddevMulThresh(std_mul)
                    sor.filter()
                    info = sor.info()
                    out["%s/sor/mean_k=%d" % (base, mean_k)] = dict(candidates=int(info["candidates"]), grown=int(info["grown"]))
                for radius, min_nb in case["ror"]:
                    for with_counts in (True, False):
                        ror.setInputCloud(case["cloud"])
                        ror.setRadiusSearch(radius)
                        ror.setMinNeighborsInRadius(min_nb)
                        ror.filter(with_counts)
                        info = ror.info()
                        out["%s/ror/r=%r/min=%d/%s" % (base, radius, min_nb, "exact" if with_counts else "early")] = dict(candidates=int(info["candidates"]),
                                                                                                                         grown=int(info["grown"]))
    finally:
        sor.setCell(0.0)
        ror.setCell(0.0)
        sor.close()
        ror.close()


def cluster_census(out):
    from rgc_slam_amd import segmentation
    ec = segmentation.EuclideanClusterExtraction(0)
    try:
        for case in cc.all_cases():
            lo, hi = case["limits"][0]
            for tol in case["tol"]:
                for cell in (tol / 8, tol, 8 * tol, 0.0):
                    ec.setCell(cell)
                    ec.setInputCloud(case["cloud"])
                    ec.setClusterTolerance(tol)
                    ec.setMinClusterSize(lo)
                    ec.setMaxClusterSize(hi)
                    ec.extract()
                    out["cluster/%s/tol=%r/cell=%g" % (case["name"], tol, cell)] = dict(candidates=int(ec.info()["candidates"]))
    finally:
        ec.setCell(0.0)
        ec.close()


def gicp_mp_census(out):
    from rgc_slam_amd import gicp
    for case in mc.all_cases():
        g = gicp.FastGICPMultiPoints(0)
        try:
            g.setCorrespondenceRandomness(case.get("k", 2 if min(len(case["tgt"]), len(case["src"])) < 20 else 20))
            g.setNeighborSearchRadius(case["r"])
            g.setInputTarget(case["tgt"])
            g.setInputSource(case["src"])
            for p, T in enumerate(case["poses"]):
                g.linearize(T, want_H=False)
                h = hashlib.sha256()
                for a in g.merged():
                    h.update(np.ascontiguousarray(a).tobytes())
                out["gicp_mp/%s/pose=%d" % (case["name"], p)] = dict(candidates=int(g.num_candidates), merged_sha256=h.hexdigest())
        finally:
            g.close()


PARTS = dict(search=search_census, outlier=outlier_census, cluster=cluster_census, gicp_mp=gicp_mp_census)


def census(parts=tuple(PARTS)):
    out = {}
    for p in parts:
        PARTS[p](out)
    return out
