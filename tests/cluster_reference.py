"""An independent numpy / scipy reference of Euclidean cluster extraction (rgc_cluster_extract, include/rgc_hip.h), and beside it a literal restatement
of PCL's algorithm (segmentation/impl/extract_clusters.hpp, from memory) for small clouds.  tests/test_cluster_reference.py shows on the CPU that the two
agree -- "a cluster is a connected component" is what PCL computes -- and what the designed cases contain; tests/test_gpu_cluster.py compares the
product with `extract` for equality.

  key        the fp32 ((dx dx + dy dy) + dz dz) in np.float32, in the product's operation order (numpy never contracts a multiply and an add)
  edges      candidate pairs from cKDTree.query_pairs in fp64 at r (1 + 1e-5) -- the key's rounding is a few 2^-24 relative, far inside that margin --
             then the strict key < r2 with r2 = float32(float64(t) float64(t))
  extract    components from scipy.sparse.csgraph.connected_components, their sizes and leaders (smallest member), the size limits, the total order
             (size descending, leader ascending), labels and CSR
  pcl_extract  seed loop over the indices, a queue grown by radius searches (brute force with the same key and rule), processed flags set for everything
             reached whether or not the cluster is kept, sort of the indices, the size test, the final order"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree


def r2_of(tolerance):
    return np.float32(float(tolerance) * float(tolerance))


def key(a, b):
    """the fp32 key of rows a against rows b (float32 arrays of x, y, z)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def candidate_pairs(cloud, tolerance):
    """(pairs (m, 2), their keys): every pair i < j the fp64 tree finds within r (1 + 1e-5)"""
    cloud = np.ascontiguousarray(cloud, np.float32)
    if len(cloud) < 2:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.float32)
    pairs = cKDTree(cloud.astype(np.float64)).query_pairs(float(tolerance) * (1.0 + 1e-5), output_type="ndarray").astype(np.int64).reshape(-1, 2)
    return pairs, key(cloud[pairs[:, 0]], cloud[pairs[:, 1]])


def extract(cloud, tolerance, min_size=1, max_size=2 ** 31 - 1):
    cloud = np.ascontiguousarray(cloud, np.float32)
    n = len(cloud)
    r2 = r2_of(tolerance)
    pairs, k = candidate_pairs(cloud, tolerance)
    e = pairs[k < r2]
    if n:
        ncomp, comp = connected_components(coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(n, n)), directed=False)
    else:
        ncomp, comp = 0, np.zeros(0, np.int64)
    sizes = np.bincount(comp, minlength=ncomp).astype(np.int64)
    leader = np.full(ncomp, n, np.int64)
    np.minimum.at(leader, comp, np.arange(n))
    kept = (sizes >= min_size) & (sizes <= max_size)
    order = np.flatnonzero(kept)
    order = order[np.lexsort((leader[order], -sizes[order]))]          # size descending, then leader ascending
    rank = np.full(ncomp, -1, np.int64)
    rank[order] = np.arange(len(order))
    labels = rank[comp].astype(np.int32) if n else np.zeros(0, np.int32)
    offsets = np.concatenate([[0], np.cumsum(sizes[order])]).astype(np.int32)
    inside = np.flatnonzero(labels >= 0)
    indices = inside[np.argsort(labels[inside], kind="stable")].astype(np.int32)   # members ascending inside a cluster
    ksz = sizes[order]
    return dict(labels=labels, offsets=offsets, indices=indices, n=n, n_components=int(ncomp), n_clusters=int(len(order)), n_clustered=int(ksz.sum()),
                largest=int(sizes.max()) if ncomp else 0, sizes=ksz, edges=int(len(e)),
                ties=int((np.bincount(ksz)[ksz] > 1).sum()) if len(ksz) else 0,             # kept clusters whose size another kept cluster shares
                over=int((sizes > max_size).sum()), under=int((sizes < min_size).sum()),
                at_r2=int((k == r2).sum()), one_under=int((k == np.nextafter(r2, np.float32(0))).sum()))


def rows(res):
    return [res["indices"][res["offsets"][r]:res["offsets"][r + 1]] for r in range(res["n_clusters"])]


def pcl_extract(cloud, tolerance, min_size=1, max_size=2 ** 31 - 1):
    """PCL's extractEuclideanClusters and the class's final sort, literally; a list of index arrays"""
    cloud = np.ascontiguousarray(cloud, np.float32)
    n = len(cloud)
    r2 = r2_of(tolerance)
    processed = np.zeros(n, bool)
    clusters = []
    for i in range(n):
        if processed[i]:
            continue
        queue = [i]
        processed[i] = True
        at = 0
        while at < len(queue):
            nb = np.flatnonzero(key(cloud[queue[at]], cloud) < r2)         # radiusSearch(queue[at], tolerance)
            at += 1
            for j in nb[~processed[nb]]:
                processed[j] = True
                queue.append(int(j))
        if min_size <= len(queue) <= max_size:
            clusters.append(np.sort(np.array(queue, np.int32)))
    clusters.sort(key=lambda c: (-len(c), int(c[0])))      # PCL: an unstable sort by size, descending; ties here by the smallest member
    return clusters
