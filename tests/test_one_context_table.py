"""The operation table of the one-context tests (tests/one_context_ops.py) against include/rgc_hip.h: every entry point that takes a context joins an
operation, or the EXCLUDED list with a reason.  A new entry point fails here until it does.  No GPU, no library."""
import os
import re

import one_context_ops as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def prototypes(text):
    """(name, argument list) of every RGC_API prototype: the regular expression of tests/fuzz/fuzz_null_args.py"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = re.findall(r"RGC_API\s+([\w\s\*]+?)\s*\b(rgc_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    return {name: [a for a in args.split(",")] if args.strip() not in ("", "void") else [] for _, name, args in protos}


def takes_a_context(args):
    return bool(args) and "rgc_ctx" in args[0]


def missing(text):
    """the entry points with a context first that are in no operation's covers and not on EXCLUDED"""
    covered = set().union(*[o.covers for o in oc.OPS.values()])
    return sorted(n for n, a in prototypes(text).items() if takes_a_context(a) and n not in covered and n not in oc.EXCLUDED)


def header():
    return open(os.path.join(ROOT, "include", "rgc_hip.h")).read()


def test_every_entry_point_with_a_context_is_in_the_table():
    assert len(prototypes(header())) > 150
    assert missing(header()) == [], "entry points in no operation of tests/one_context_ops.py (add them to an operation's covers, or to EXCLUDED with a reason)"


def test_a_new_entry_point_is_missed():
    """the check can fail: a prototype added to the header's text, and an operation taken out of the table"""
    assert missing(header() + "\nRGC_API int rgc_x(rgc_ctx* ctx);\n") == ["rgc_x"]
    assert missing(header() + "\nRGC_API int rgc_no_context(int a);\n") == []
    op = oc.OPS.pop("cluster_extract")
    try:
        assert missing(header()) == ["rgc_cluster_extract", "rgc_cluster_get_info"]
    finally:
        oc.OPS[op.name] = op


def test_covers_and_exclusions_name_real_entry_points():
    protos = prototypes(header())
    for o in oc.OPS.values():
        assert o.covers and o.covers <= set(protos), (o.name, sorted(o.covers - set(protos)))
        assert all(takes_a_context(protos[n]) for n in o.covers), o.name
    for n, why in oc.EXCLUDED.items():
        assert n in protos and takes_a_context(protos[n]) and why.strip(), n
    covered = set().union(*[o.covers for o in oc.OPS.values()])
    assert not covered & set(oc.EXCLUDED), sorted(covered & set(oc.EXCLUDED))


def test_every_operation_is_complete():
    for o in oc.OPS.values():
        assert set(o.sizes) == set(oc.SIZES) and all(isinstance(v, str) and v for v in o.sizes.values()), o.name
        assert o.in_flight in ("refused", "runs") and o.forms and set(o.forms) <= {"host", "device"}, o.name
        assert o.reads <= set(oc.GROUPS) and o.writes <= set(oc.GROUPS) and o.reads <= o.writes, o.name
        assert callable(o.make) and callable(o._run), o.name
        assert (o.begin is None) == (o.end is None), o.name
        assert bool(o.reads) == (o._kept is not None), o.name


def test_large_has_four_times_the_points_of_small():
    """`large` makes every ensure() reallocate behind `small`: at least four times the points, but for the entries that say EXCEPTION and why"""
    for o in oc.OPS.values():
        small, large = oc.points(o.make("small")), oc.points(o.make("large"))
        assert small > 0 and (large >= 4 * small or "EXCEPTION" in o.sizes["large"]), (o.name, small, large)


def test_the_families_the_table_must_hold():
    need = ["rgc_set_target", "rgc_align", "rgc_align_begin", "rgc_align_end", "rgc_get_aligned", "rgc_get_voxels", "rgc_set_rbf_kernel", "rgc_gicp_align", "rgc_gicpst_align",
            "rgc_gicpmp_align", "rgc_gicp_linearize", "rgc_gicp_compute_error", "rgc_ndt_align", "rgc_search_set_cloud", "rgc_search_knn", "rgc_search_radius",
            "rgc_outlier_statistical", "rgc_outlier_radius", "rgc_cluster_extract", "rgc_plane_segment", "rgc_normal_estimate", "rgc_fpfh_estimate", "rgc_voxelgrid",
            "rgc_voxelgrid_begin", "rgc_voxelgrid_end", "rgc_uniform_sampling", "rgc_deskew", "rgc_transform_cloud", "rgc_frontend", "rgc_kf_push", "rgc_kf_set_poses",
            "rgc_kf_assemble", "rgc_kf_select_surrounding", "rgc_kf_select_global", "rgc_kf_detect_loop", "rgc_pgo_linearize", "rgc_pgo_optimize", "rgc_map_insert",
            "rgc_map_commit", "rgc_map_evict", "rgc_map_rebase", "rgc_icp_align", "rgc_icp_align_device", "rgc_mapreg_optimize", "rgc_pc2_unpack", "rgc_pc2_pack"]
    covered = set().union(*[o.covers for o in oc.OPS.values()])
    assert [n for n in need if n not in covered] == []


def test_in_flight_is_what_the_header_says():
    """the sentences the in_flight column is copied from are in the header"""
    text = " ".join(header().split())
    for sentence in ("new clouds, clearing or swapping them, another begin or a blocking rgc_align, the settings that re-route a cloud, the getters",
                     "With a solve in flight (rgc_align_begin .. rgc_align_end) every one of them RUNS",
                     "a solve in flight refuses its calls (RGC_ERR_INVALID)",
                     "Everything else RUNS with a solve in flight"):
        assert " ".join(sentence.split()) in text.replace(" * ", " "), sentence
