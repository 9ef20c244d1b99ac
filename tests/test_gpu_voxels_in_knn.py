"""The voxel map built INSIDE the dense map's kNN launch (RGC_VOXEL_IMPL=fused; unset, the choice of a context of a pipelined sequence,
whose scans are held behind the other context's target -- test_dependent_sequence_on_two_contexts: every workgroup of k_knn_sp writes the voxel records of its own cells,
the launch's last workgroups resolve the deferred queries, k_voxel_seams finishes the cells that cross a workgroup boundary and the voxels
of the deferred queries) against the stages in launches of their own (RGC_VOXEL_IMPL=separate: k_voxel_build_coop + k_voxel_patch).  Every
sum keeps its order, so every comparison here is == on bytes, no tolerance anywhere.  Needs an MI355X: -m gpu.

A workgroup of the search takes 256 consecutive points of the sorted order (cell by cell, x fastest, then y, then z; a cell's points in
the cloud's order), so the maps below are designed cell by cell: a point at integer coordinates +- 0.45 lies in the 1 m cell around them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FUSED = "fused"  # (a context by itself keeps the stages apart unless told otherwise: its scan is prepared beside its map's search)
ROUTES = (FUSED, "separate")


@pytest.fixture(scope="module")
def reg_mod():
    from rgc_slam_amd import registration
    return registration


def _ctx(reg_mod, monkeypatch, impl, k=20):
    """a context of the given route (the environment is read when the context is created), 1 m voxels"""
    if impl is None:
        monkeypatch.delenv("RGC_VOXEL_IMPL", raising=False)
    else:
        monkeypatch.setenv("RGC_VOXEL_IMPL", impl)
    v = reg_mod.odometer_vgicp(0)
    monkeypatch.delenv("RGC_VOXEL_IMPL", raising=False)
    v.setResolution(1.0)
    if k != 20:
        v.setCorrespondenceRandomness(k)
    return v


def _cells(spec, seed=7, shuffle=True):
    """spec: [((cx, cy, cz), count)] -> float32 points, `count` of them in the cell around each centre"""
    rng = np.random.default_rng(seed)
    pts = [np.asarray(c, np.float64) + rng.uniform(-0.45, 0.45, (m, 3)) for c, m in spec]
    p = np.concatenate(pts).astype(np.float32)
    return p[rng.permutation(len(p))] if shuffle else p


def _box(dims, counts):
    """the cells of an (nx, ny, nz) box in sorted order (x fastest), counts[j] points in the j-th (a number: in every one)"""
    nx, ny, nz = dims
    cen = [(x + 1, y + 1, z + 1) for z in range(nz) for y in range(ny) for x in range(nx)]
    if np.isscalar(counts):
        counts = [counts] * len(cen)
    assert len(counts) == len(cen)
    return list(zip(cen, counts))


def _uniform(n, dims, seed=3):
    """n points spread evenly over the box's cells: about ten a cell, every cell occupied"""
    ncell = dims[0] * dims[1] * dims[2]
    counts = [n // ncell + (1 if j < n % ncell else 0) for j in range(ncell)]
    return _cells(_box(dims, counts), seed)


DIMS = {255: (3, 3, 3), 256: (3, 3, 3), 257: (3, 3, 3), 511: (4, 4, 3), 512: (4, 4, 3), 513: (4, 4, 3), 600: (4, 4, 4), 2000: (6, 6, 5)}


def _scan_of(tgt):
    import rgc_slam_amd.synth as synth
    M = synth.se3(synth.rot_zyx(0.01, 0.002, -0.001), [0.05, -0.03, 0.01])
    return (tgt[::2].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)


def _map_state(v):
    vox = v.getVoxels()
    return dict(coords=vox["coords"].tobytes(), num=vox["num"].tobytes(), mean=vox["mean"].tobytes(), cov=vox["cov"].tobytes(),
                normals=v.getTargetNormals().tobytes())


def _solve_state(v, tgt):
    v.setInputSource(_scan_of(tgt))
    v.align(np.eye(4), want_output=False)
    return dict(T=v.getFinalTransformation().tobytes(), H=v.getFinalHessian().tobytes(), fit=np.float64(v.getFitnessScore()).tobytes(),
                stats=v.stats())


def _on_the_dense_launch(st, deferred):
    assert st["n_target"] >= 0.25 * st["target_cells"], st  # the dense launch (not the sparse map's wide block)
    if deferred is not None:
        assert (st["deferred_target"] > 0) if deferred else (st["deferred_target"] == 0), st


def _target_state(v, tgt, deferred):
    v.setInputTarget(tgt)
    out = _map_state(v)
    out.update(_solve_state(v, tgt))
    print(len(tgt), {k: out["stats"][k] for k in ("n_target", "target_cells", "n_voxels", "deferred_target", "n_corr")})
    _on_the_dense_launch(out["stats"], deferred)
    return out


def _both(reg_mod, monkeypatch, tgt, deferred, k=20):
    res = {}
    for impl in ROUTES:
        v = _ctx(reg_mod, monkeypatch, impl, k)
        res[impl] = _target_state(v, tgt, deferred)
        v.close()
    return res


def _same(res):
    a, b = res[FUSED], res["separate"]
    assert [key for key in a if a[key] != b[key]] == []


@pytest.mark.parametrize("n", [255, 256, 257, 511, 512, 513, 2000])
def test_block_edges(reg_mod, monkeypatch, n):
    """one workgroup short of a block, exactly one, one point into the second, the same around two blocks, several blocks"""
    _same(_both(reg_mod, monkeypatch, _uniform(n, DIMS[n]), None))


def test_cells_that_end_on_a_blocks_end(reg_mod, monkeypatch):
    """32 cells of 16 points: sorted position 256 starts a cell, no cell crosses a boundary -- the seam waves find nothing to do"""
    _same(_both(reg_mod, monkeypatch, _cells(_box((4, 4, 2), 16)), None))


def test_a_cell_straddling_position_256(reg_mod, monkeypatch):
    """15 cells of 16 points, then one of 40: sorted positions 240 .. 279"""
    counts = [16] * 32
    counts[15] = 40
    _same(_both(reg_mod, monkeypatch, _cells(_box((4, 4, 2), counts)), None))


def test_a_cell_across_three_blocks(reg_mod, monkeypatch):
    """4 cells of 16 points, then one of 700: sorted positions 64 .. 763, boundaries 256 and 512, one owner (the first boundary).  Its
    rows hold more than 128 candidates, so every query near it is deferred: the neighbours' voxels are the patch waves' work."""
    counts = [16] * 32
    counts[4] = 700
    res = _both(reg_mod, monkeypatch, _cells(_box((4, 4, 2), counts)), True)
    assert res[FUSED]["stats"]["deferred_target"] >= 700
    _same(res)


def _with_lone_cell(before, lone):
    """a slab of 16 cells holding `before` points (z = 1), a lone cell of `lone` points three layers above it (no neighbour in its 3x3x3
    block: its queries are deferred) at sorted positions before .. before + lone - 1, and a second slab three layers above that"""
    counts = [before // 16 + (1 if j < before % 16 else 0) for j in range(16)]
    spec = _box((4, 4, 1), counts) + [((2, 2, 4), lone)] + [((x + 1, y + 1, 7), 17) for y in range(4) for x in range(4)]
    return _cells(spec)


@pytest.mark.parametrize("before,lone", [(254, 4), (256, 3), (253, 3)], ids=["in_a_seam_cell", "a_blocks_first_point", "a_blocks_last_point"])
def test_deferred_queries_at_a_boundary(reg_mod, monkeypatch, before, lone):
    res = _both(reg_mod, monkeypatch, _with_lone_cell(before, lone), True)
    assert res[FUSED]["stats"]["deferred_target"] >= lone
    _same(res)


def test_deferred_queries_in_the_far_field(reg_mod, monkeypatch):
    """a dense slab and a sparse fringe three cells off it: three deferred queries share each fringe voxel"""
    spec = _box((6, 6, 2), 10) + [((10, y + 1, 1), 3) for y in range(0, 6, 2)]
    res = _both(reg_mod, monkeypatch, _cells(spec), True)
    assert res[FUSED]["stats"]["deferred_target"] >= 9
    _same(res)


def test_a_map_without_deferred_queries(reg_mod, monkeypatch):
    """18 points a cell in a box whose faces are the grid's borders: every block proves its 20th neighbour, no row exceeds 128 candidates;
    cells cross the boundaries at 256 and 512"""
    _same(_both(reg_mod, monkeypatch, _cells(_box((4, 4, 2), 18), seed=11), False))


@pytest.mark.parametrize("k", [10, 25])
def test_other_k(reg_mod, monkeypatch, k):
    """the general-k instance (KC = 20) and the KC = 32 one"""
    _same(_both(reg_mod, monkeypatch, _uniform(2000, DIMS[2000]), None, k=k))


MAP_KEYS = ("coords", "num", "mean", "cov", "normals")


def test_slots_clean_between_targets(reg_mod, monkeypatch):
    """one context, three targets in a row: the deferred list's entry words are as the next launch needs them.  Each map equals the same
    target's on a fresh context; the solves (a context steers its next scan's grid by the last one's crowding, so a solve depends on the
    context's history) equal those of the same three targets in a row on the other route."""
    maps = [_uniform(2000, DIMS[2000]), _uniform(600, DIMS[600], seed=5), _uniform(2000, DIMS[2000])]
    fresh = []
    for m in maps[:2]:
        v = _ctx(reg_mod, monkeypatch, FUSED)
        fresh.append(_target_state(v, m, True))
        v.close()
    fresh.append(fresh[0])
    row = {}
    for impl in ROUTES:
        v = _ctx(reg_mod, monkeypatch, impl)
        row[impl] = [_target_state(v, m, True) for m in maps]
        v.close()
    for got, ref in zip(row[FUSED], fresh):
        # (which queries are deferred depends on the grid the context re-uses, and the scan's grid -- hence the order the solve's sums take its
        # points in, the last bits of H: measured, one ulp, on either route alike -- on the crowding of the context's previous scan)
        assert [key for key in MAP_KEYS if got[key] != ref[key]] == []
    assert row[FUSED] == row["separate"]


def test_a_larger_target_in_the_same_allocation(reg_mod, monkeypatch):
    """300 points, then 400: the second target's deferred list fits the head-room of the first one's buffer, so its entry words beyond the
    first target's are as the allocation's one fill left them"""
    maps = [_uniform(300, DIMS[257], seed=9), _uniform(400, DIMS[511], seed=9)]
    row = {}
    for impl in ROUTES:
        v = _ctx(reg_mod, monkeypatch, impl)
        row[impl] = [_target_state(v, m, None) for m in maps]
        v.close()
    assert row[FUSED] == row["separate"]


_SEQ = {}


def _sequence(reg_mod, monkeypatch, impl, reuse):
    """the path the headline runs: six dependent frames, align_begin / align_end_reframe on two contexts taking turns, a 20 000-point map
    and 2 000-point scans -> (motions, world poses, lm_fallbacks and deferred_target of the two contexts); computed once per configuration"""
    import bench
    import rgc_slam_amd.synth as synth
    if (impl, reuse) in _SEQ:
        return _SEQ[(impl, reuse)]
    if "data" not in _SEQ:
        world, tgt = synth.make_world_and_map(20000, seed=synth.SEED)
        scans = []
        for i in range(6):
            M = synth.se3(synth.rot_zyx(0.02 + 0.004 * i, 0.002 - 0.001 * i, -0.001 + 0.0005 * i), [0.12 + 0.03 * i, 0.02 - 0.01 * i, 0.001 + 0.002 * i])
            scans.append(synth.make_scan_n(world, M, 2000, seed=synth.SEED + i)["xyz"].astype(np.float32))
        _SEQ["data"] = (tgt, scans)
    tgt, scans = _SEQ["data"]
    ctxs = [_ctx(reg_mod, monkeypatch, impl), _ctx(reg_mod, monkeypatch, impl)]
    for w in ctxs:
        w.setNeighbourReuse(reuse)
    pv = reg_mod.PipelinedVGICP(0, depth=2, contexts=ctxs)
    v = pv.v[0]

    def to_dev(xyz):
        a = np.zeros((xyz.shape[0], 4), np.float32)
        a[:, :3] = xyz
        p = v.device_alloc(a.nbytes)
        v.upload(p, a)
        return p
    d_map, d_scans = to_dev(tgt), [to_dev(s) for s in scans]
    seq = bench.DependentSequence(pv.v, d_map, len(tgt), d_scans, [len(s) for s in scans])
    motions, worlds, _ = seq.run(0, 6, np.eye(4), np.eye(4, dtype=np.float32), True)
    st = [w.stats() for w in pv.v]
    for s_ in st:
        assert s_["n_target"] >= 0.25 * s_["target_cells"], s_
    out = ([m.tobytes() for m in motions], [w.tobytes() for w in worlds], [s_["lm_fallbacks"] for s_ in st], [s_["deferred_target"] for s_ in st])
    seq.close()
    for p in [d_map] + d_scans:
        v.device_free(p)
    for w in pv.v:
        w.close()
    _SEQ[(impl, reuse)] = out
    return out


def test_dependent_sequence_on_two_contexts(reg_mod, monkeypatch):
    """nothing kept between the frames' targets (REUSE_NONE, the headline's setting): every frame's map takes the dense launch in full"""
    R = reg_mod.FastVGICP
    got, ref = _sequence(reg_mod, monkeypatch, None, R.REUSE_NONE), _sequence(reg_mod, monkeypatch, "separate", R.REUSE_NONE)
    print("deferred_target", got[3])
    assert len(got[0]) == 6 and got[3][0] > 0
    assert got == ref


def test_the_neighbour_list_cache_unchanged(reg_mod, monkeypatch):
    """REUSE_LISTS: from the second frame on the maps take the seeded kernel and the lists, which keep the voxel stage's own launches --
    and give the fused sequence's poses bit for bit"""
    R = reg_mod.FastVGICP
    got, ref = _sequence(reg_mod, monkeypatch, None, R.REUSE_LISTS), _sequence(reg_mod, monkeypatch, None, R.REUSE_NONE)
    assert got[:3] == ref[:3]


def test_the_lazy_target_unchanged(reg_mod, monkeypatch):
    """a lazy target (the listed queries' kernel, the voxel pass over the listed cells) beside a fused context, two targets in a row on each
    (the second meets what the first one left in the deferred list's words): the same map, the same solve"""
    tgt = _uniform(2000, DIMS[2000])
    res = {}
    for lazy in (0, 2):
        v = _ctx(reg_mod, monkeypatch, FUSED)
        v.setLazyTarget(lazy)
        res[lazy] = []
        for rep in range(2):
            v.setInputTarget(tgt)
            s = _solve_state(v, tgt)
            s.update(_map_state(v))  # (read behind the solve: completes a lazy target)
            res[lazy].append(s)
        v.close()
    for got, ref in zip(res[2], res[0]):
        assert [key for key in ("T", "H", "fit") + MAP_KEYS if got[key] != ref[key]] == []
        assert [key for key in ("n_target", "n_voxels", "n_corr", "outer_iterations", "target_cells") if got["stats"][key] != ref["stats"][key]] == []
