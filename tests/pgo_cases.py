"""Designed pose graphs for the rgc_pgo_* tests.  Every case is built from numpy alone and DECLARES what it exercises, from the reference alone
(tests/pgo_reference.py): tests/test_pgo_reference.py asserts the declared minima without a GPU, tests/test_gpu_pose_graph.py runs the library on
the same cases.  A case: dict(store_ids, store_poses (float32), ids (the selection, in the caller's order), loops, params, expect)."""
import functools

import numpy as np

import pgo_reference as ref

SEGMENT = 32      # the builder's segment size for selections of up to 32 * 96 keyframes (rgc_api_pgo.hip: kPgoMinSegment)
RHO_MARGIN = 4.0          # every rho is outside [1e-3 / RHO_MARGIN, 1e-3 * RHO_MARGIN]
FTOL_MARGIN = 2.0         # every accepted step's relative cost change is outside [1e-6 / FTOL_MARGIN, 1e-6 * FTOL_MARGIN]
PTOL_MARGIN = 10.0        # every accepted step's norm is above 1e-8 * PTOL_MARGIN * (|x| + 1e-8): the parameter tolerance never decides


def trajectory(n, seed, step=1.0, turn_deg=4.0, yaw0_deg=20.0, tilt_deg=4.0):
    """n key poses (float32 x, y, z, roll, pitch, yaw [rad]) of a drive: ~`step` metres and ~`turn_deg` degrees between neighbours, pitch and
    roll of several degrees, the yaw kept in (-180, 180]"""
    rng = np.random.default_rng(seed)
    yaw = np.deg2rad(yaw0_deg) + np.cumsum(np.deg2rad(turn_deg) * (1.0 + 0.3 * rng.standard_normal(n)))
    yaw = (yaw + np.pi) % (2 * np.pi) - np.pi
    d = step * (1.0 + 0.2 * rng.standard_normal(n))
    xy = np.cumsum(np.stack([d * np.cos(yaw), d * np.sin(yaw)], 1), 0)
    z = np.cumsum(0.05 * rng.standard_normal(n))
    pitch = np.deg2rad(tilt_deg) * rng.standard_normal(n)
    roll = np.deg2rad(tilt_deg) * rng.standard_normal(n)
    return np.stack([xy[:, 0], xy[:, 1], z, roll, pitch, yaw], 1).astype(np.float32)


def loop_between(ids, poses, key_curr, key_loop, rng, err_t=0.3, err_yaw=3.0, err_tilt=0.5):
    """a loop edge key_loop -> key_curr: the relative pose the stored poses themselves give, plus an error of decimetres and degrees (so that the
    residuals are macroscopic); pitch / roll: the loop pose's "as recorded at detection", a little off the stored ones"""
    pos = {k: i for i, k in enumerate(ids)}
    x, pitch, roll = ref.state_of(poses)
    a, b = pos[key_loop], pos[key_curr]
    R, _ = ref.ypr_matrix(x[a, 0], pitch[a], roll[a], np.float64)
    t = R.T @ (x[b, 1:4] - x[a, 1:4]) + err_t * rng.standard_normal(3)
    yaw = ref.normalize_angle(ref.normalize_angle(x[b, 0] - x[a, 0]) + err_yaw * rng.standard_normal())
    return dict(key_curr=int(key_curr), key_loop=int(key_loop), t=t, yaw=float(yaw), pitch=float(pitch[a] + err_tilt * rng.standard_normal()),
                roll=float(roll[a] + err_tilt * rng.standard_normal()))


def _case(name, n_store, pairs, seed, select=None, id_of=None, params=None, expect=None, traj=None, loop_err=None, extra_loops=()):
    ids_store = [int(id_of(i)) if id_of else i for i in range(n_store)]
    poses = trajectory(n_store, seed, **(traj or {}))
    sel = list(range(n_store)) if select is None else list(select)
    ids = [ids_store[i] for i in sel]
    rng = np.random.default_rng(seed + 1000)
    loops = [loop_between(ids_store, poses, ids_store[c], ids_store[l], rng, **(loop_err or {})) for c, l in pairs] + list(extra_loops)
    return dict(name=name, store_ids=ids_store, store_poses=poses, ids=ids, sel_poses=poses[sel], loops=loops, params=dict(params or {}), expect=dict(expect or {}))


def _big_pairs(n_nodes, n_loops, seed):
    rng = np.random.default_rng(seed)
    pairs = set()
    while len(pairs) < n_loops:
        a, b = sorted(int(v) for v in rng.integers(1, n_nodes, 2))
        if b - a >= 2:
            pairs.add((b, a))
    return sorted(pairs)


@functools.lru_cache(maxsize=None)
def cases():
    """every case, by name.  expect: status, fixed (position), n_used, n_ignored, refused, and the LM path's minima: stop, min_rejected"""
    S = SEGMENT
    sparse = lambda i: 3 * i + 11                                                    # noqa: E731  non-contiguous ids
    out = [
        _case("n1_no_loop", 1, [], 1, expect=dict(status=ref.NO_LOOP)),
        _case("n2_neighbours", 2, [(1, 0)], 2, expect=dict(fixed=0, n_used=1, neighbour_loop=True, loop_onto_fixed=True)),
        _case("n3_fixed_middle", 3, [(2, 1)], 3, id_of=lambda i: [70, 30, 90][i], expect=dict(fixed=1, n_used=1, neighbour_loop=True)),
        _case("one_loop", 40, [(39, 0)], 4, expect=dict(fixed=0, n_used=1, loop_onto_fixed=True, stop="function")),
        _case("fixed_last", 24, [(5, 23)], 5, expect=dict(fixed=23, n_used=1)),                  # the edge runs backwards: i > j
        _case("shared_node", 48, [(40, 3), (40, 17), (30, 3)], 6, id_of=sparse, expect=dict(fixed=3, n_used=3)),
        _case("nested_crossing", 60, [(40, 5), (30, 10), (50, 20), (21, 20)], 7, expect=dict(fixed=5, n_used=4, neighbour_loop=True)),
        # a strict subset of the store; one loop's id is not selected, one ends at position 0
        _case("ignored", 50, [(45, 8), (47, 49), (4, 30)], 8, select=[4] + list(range(5, 48)), id_of=sparse, expect=dict(fixed=4, n_used=1, n_ignored=2)),
        _case("only_ignored", 12, [(0, 7)], 9, expect=dict(status=ref.NO_LOOP, n_ignored=1)),
        _case("wrap", 36, [(29, 3), (20, 6)], 10, traj=dict(turn_deg=14.0, yaw0_deg=150.0), expect=dict(fixed=3, n_used=2, yaw_wrap=True)),
        _case("seg_S-1", S - 1, [(S - 2, 3)], 11, expect=dict(fixed=3, n_used=1)),
        _case("seg_S", S, [(S - 1, 3)], 12, expect=dict(fixed=3, n_used=1)),
        _case("seg_S+1", S + 1, [(S, 3)], 13, expect=dict(fixed=3, n_used=1)),
        _case("seg_2S+1", 2 * S + 1, [(2 * S, 3), (S + 5, S - 5)], 14, expect=dict(fixed=3, n_used=2)),
        _case("big_100_on_300", 300, _big_pairs(300, 100, 15), 15, expect=dict(n_used=100)),
        _case("refused_129", 300, _big_pairs(300, 129, 16), 16, expect=dict(refused=True)),
        _case("cap_2", 40, [(39, 0), (25, 8)], 17, params=dict(max_iterations=2), expect=dict(fixed=0, n_used=2, stop="cap", iterations=2)),
    ]
    out += _lm_cases()
    return {c["name"]: c for c in out}


def _lm_cases():
    """the rejected-step path, found by a bounded search with the reference alone (EXPERIMENTS.md "Round 15" has its size).  Loop errors of decimetres
    and degrees, and of up to 60 m and 120 degrees on 60 m edges, kept rho in 0.33 .. 1.5: the problem is nearly linear.  What rejects a step is a
    long lever arm: keyframes hundreds of metres apart and two loops that are off by as much and by ~150 degrees, started at a radius where
    the step is the Gauss-Newton step -- the rotation of such an edge by tens of degrees is far from its linearisation."""
    out = []
    for name, seed, step in REJECTED_CASES:
        rng = np.random.default_rng(seed)
        base = _case(name, 30, [], seed, traj=dict(turn_deg=10.0, step=step))
        ids, poses = base["store_ids"], base["store_poses"]
        loops = [loop_between(ids, poses, 29, 1, rng, err_t=step, err_yaw=150.0), loop_between(ids, poses, 17, 5, rng, err_t=step, err_yaw=150.0)]
        base.update(loops=loops, params=dict(initial_radius=1e16), expect=dict(fixed=1, n_used=2, min_rejected=1, min_accepted=1, stop="cap"))
        out.append(base)
    return out


# (name, seed, metres between keyframes): see _lm_cases
REJECTED_CASES = [("rejected_then_accepted", 1, 1000.0), ("accepted_then_rejected", 6, 200.0)]


def reference_graph(case):
    return ref.build_graph(case["ids"], case["sel_poses"], case["loops"])


@functools.lru_cache(maxsize=None)
def reference_solve(name):
    """the reference's LM run of a case (computed once, shared): (graph, x0, x, info)"""
    c = cases()[name]
    g = reference_graph(c)
    x0, _, _ = ref.state_of(c["sel_poses"])
    x, info = ref.lm_solve(g, x0, c["params"].get("max_iterations", 10), c["params"].get("initial_radius", 1e4))
    return g, x0, x, info


def perturbed(case, seed=0, dt=0.4, dyaw=2.5):
    """a state off the store's, where every residual is macroscopic"""
    x0, _, _ = ref.state_of(case["sel_poses"])
    rng = np.random.default_rng(1234 + seed)
    x = x0 + np.concatenate([dyaw * rng.standard_normal((len(x0), 1)), dt * rng.standard_normal((len(x0), 3))], 1)
    x[:, 0] = [ref.normalize_angle(v) for v in x[:, 0]]
    return x


def check_margins(info):
    """no decision of this LM run hangs on the last bits"""
    for s in info["steps"]:
        assert not (1e-3 / RHO_MARGIN <= s["rho"] <= 1e-3 * RHO_MARGIN), s
        if s["accepted"]:
            assert not (1e-6 / FTOL_MARGIN <= s["dcost"] <= 1e-6 * FTOL_MARGIN), s
            if s["dcost"] > 1e-6:      # the function tolerance is tested first: where it stops the run the parameter tolerance is not asked
                assert s["step_norm"] > PTOL_MARGIN * 1e-8 * (s["x_norm"] + 1e-8), s


SOLVE_CASES = ["n2_neighbours", "n3_fixed_middle", "one_loop", "fixed_last", "shared_node", "nested_crossing", "ignored", "wrap", "seg_S-1", "seg_S", "seg_S+1",
               "seg_2S+1", "big_100_on_300", "cap_2"] + [n for n, _, _ in REJECTED_CASES]
TERM_CASES = [n for n in SOLVE_CASES if n != "big_100_on_300"] + ["big_100_on_300"]


# ---- the two bars of tests/test_gpu_pose_graph.py, measured without a GPU (tests/test_pgo_reference.py prints them) --------------------------
STEP_STATES = ("initial", "perturbed")


def eval_state(name, which):
    c = cases()[name]
    return ref.state_of(c["sel_poses"])[0] if which == "initial" else perturbed(c)


@functools.lru_cache(maxsize=None)
def reference_eval(name, which):
    """the longdouble evaluation of a case at its initial or its perturbed state, on the reference's own edge table"""
    return ref.evaluate(reference_graph(cases()[name]), eval_state(name, which), ref.LD)


def step_radii(name):
    return (cases()[name]["params"].get("initial_radius", 1e4), 1e16)


def step_states(name):
    return STEP_STATES


@functools.lru_cache(maxsize=None)
def reference_step(name, which, radius):
    return ref.step_ld(reference_graph(cases()[name]), reference_eval(name, which), radius)


@functools.lru_cache(maxsize=None)
def _fp64_deviations():
    """per case: the deviation (|difference| / sum |terms|) of the plain sequential fp64 numpy evaluation from the longdouble reference at the perturbed
    state, and the largest max |d - d_ref| / max |d_ref| of np.linalg.solve in fp64 on the same damped systems from the longdouble Cholesky over
    the case's states and both radii"""
    term, step = {}, {}
    for name in TERM_CASES:
        g = reference_graph(cases()[name])
        x = eval_state(name, "perturbed")
        term[name], zeros = ref.term_deviation(g, x, ref.fp64_readout(g, x), reference_eval(name, "perturbed"))
        assert zeros, name
        step[name] = max(ref.step_deviation(ref.step_fp64(g, reference_eval(name, which), radius), reference_step(name, which, radius))
                         for which in step_states(name) for radius in step_radii(name))
    return term, step


# The issue's bar is 8 x the largest fp64 deviation over ALL cases.  The two LM-path cases with keyframes hundreds of metres apart set that
# maximum alone (their residuals cancel from kilometres to decimetres: 2e-13 on the terms, 2e-11 on the step, against 2e-14 and 5e-14 on every
# other case), and a bar taken from them would let the metre-scale cases pass with errors a thousand times their fp64 noise.  So a
# metre-scale case is held to 8 x the largest deviation among the metre-scale cases, a long-lever case to 8 x the largest of all: never wider
# than the issue's bar.
LONG_LEVER = tuple(n for n, _, _ in REJECTED_CASES)


def term_bar(name=None):
    term, _ = _fp64_deviations()
    return 8.0 * max(v for n, v in term.items() if name in LONG_LEVER or name is None or n not in LONG_LEVER)


def step_bar(name=None):
    _, step = _fp64_deviations()
    return 8.0 * max(v for n, v in step.items() if name in LONG_LEVER or name is None or n not in LONG_LEVER)
