#!/usr/bin/env python3
"""bench.py -- registered scans/s of the HIP scan-to-map registration path (BASELINE.json metric).

One "step" = one frame of a DEPENDENT sequence, as the reference's odometer runs it (RGC_odometer.cpp:976-1256): the 1 M-point local
map is re-expressed in the body frame of the pose the previous step returned (B9, :1248-1256, on the device), handed to the registration
as a new target -- covariances + Gaussian voxel map rebuilt from scratch, the reference re-creates FastVGICP every frame (:998) -- the next
synthetic VLP-16 scan (30 k points) is the source, the guess is the previous step's motion, and the step ends with the LM solve + fitness
and the new world pose.  Step i + 1's TARGET depends on step i's result, so only the next scan's preparation can run under a solve: that
is what the two contexts of `value` overlap.  Inputs (the map in the world frame, the scans) are resident in HBM before the timed
region starts.

`value` is timed with rgc_set_knn_reuse(RGC_REUSE_NONE): every step's target is searched like a map the library has NOT seen before --
the full exact 20-NN of all 1 M points, no state of any kind carried from step to step.  That is what the reference does and what a
drop-in caller of this path pays: the reference pushes the re-framed sub-map through a pcl::VoxelGrid in the new body frame before
setInputTarget (RGC_odometer.cpp:985-991, 1007), so its target is a new point set every frame.  The library's default (seeds +
neighbour lists of a map it can verify to be bit for bit last frame's) is faster on THIS synthetic sequence, whose world-frame map never
changes; that figure is the extra key `reuse_of_an_unchanged_map`, beside `one_point_edited_every_frame` and
`keyframe_every_3rd_frame` (what it gives when the map does change), each timed exactly like `value`.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full [--configs c1,c3,c5]]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the headline (`value`, `ms_per_step`, the workload); --dump-outputs DIR
also writes the last timed step's motion, world pose, fitness and iteration count as DIR/<name>.npy (rank r > 0: <name>_rank<r>.npy).
The inputs depend on the arguments only (seeded).  A sequence has at most SCAN_POOL distinct scans: a longer one goes forth and back
over the first SCAN_POOL poses of its trajectory (scan_schedule), so that the setup does not grow with K.  Everything else below --
the extra keys, the CPU baseline and parity check, the other configurations -- runs with --full only.

N > 1: one process per GPU, one independent sequence per rank (different seed), no data-path collective
(the path shards across sequences); torch.distributed (RCCL) is used only for the barrier and the
MAX over ranks of the elapsed time.  Rank 0 prints ONE JSON line.

Extra keys beside the contract's (--full): `one_frame_at_a_time` (the same steps on one context through the blocking calls: a frame's latency),
`replay_of_preframed_maps` (round 2's figure: targets that do NOT depend on the previous pose -- three translated copies of the map in
turn -- so that a whole frame's preparation overlaps the previous solve; what a replay of pre-framed sub-maps reaches, not a live
sequence), `scan_h2d_and_output` (the dependent steps with each scan uploaded from pinned host memory inside the step and align()'s
output cloud produced on the device), `steady_state` (the K timed steps repeated ten times back to back without HIP events in the
loop: what a sequence that keeps running sustains), `issue_roofline` (the dominant kernel against the measured VALU issue rates), `configs`
(BASELINE.json's other single-GPU configurations, a few frames each, with their own hbm_frac_whole_frame), `roofline_by_kernel` (the five
kernels that take the most GPU time in a frame of the timed workload, each against its own algorithmic bytes and its measured traffic),
`sequences_per_gpu` (S = 1, 2, 4, 8 independent sequences on ONE GPU driven by a C++ host thread each: what one GPU can carry).
"""
import argparse
import gc
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_SOURCE = 30000
N_TARGET = 1000000
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md
MAP_SHIFTS = ((0.0, 0.0, 0.0), (0.37, -0.23, 0.011), (-0.29, 0.41, -0.007))  # m: the map copies `replay_of_preframed_maps` alternates between
# Constants of this line that are NOT measured in this run: they are read from committed profile summaries (separate rocprofv3 --pmc passes
# cannot run inside a timed bench) and every one is stamped with its file and the commit it was collected at (`*_source` keys): a kernel
# change that was not followed by scripts/refresh_profiles.sh shows up as a stale stamp, not as a silently wrong number.
PMC_FILE = "r06_pmc_knn.json"      # counters of the dominant kernel (scripts/pmc_seeded.sh): top level = the launch `value` runs (full search)
MIX_FILE = "r06_knn_isa_mix.json"  # its full- / half-rate instruction mix (scripts/isa_mix.py)
FRAME_TRAFFIC_FILE = "r06_frame_traffic.json"  # measured HBM bytes of a whole dependent frame, every kernel (scripts/frame_traffic.sh)
KERNEL_STATS_FILE = "r06_frame_kernel_times.json"  # GPU time per kernel and frame of the timed workload under rocprofv3 (scripts/frame_kernel_times.sh)
REUSE_NONE, REUSE_SEEDS, REUSE_LISTS = 0, 1, 2   # rgc_set_knn_reuse
SCAN_POOL = 128    # distinct synthetic scans of a sequence (make_sequence): longer sequences go forth and back over them


def profile_json(name):
    """(contents, source stamp) of a committed profile summary, or (None, None)"""
    path = os.path.join(ROOT, "profiles", name)
    if not os.path.exists(path):
        return None, None
    try:
        d = json.load(open(path))
    except Exception:
        return None, None
    return d, f"profiles/{name}@{d.get('commit') or 'unstamped'}"


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def algorithmic_bytes(n_s, n_t, n_vox, n_corr, n_lin, n_err):
    """SURVEY.md §8d yardstick (fixed; fused stages may not shrink it)."""
    return 36.0 * n_s + 36.0 * n_t + (36.0 * n_t + 40.0 * n_vox) + (n_lin + n_err) * (36.0 * n_s + 40.0 * n_corr) + 24.0 * n_s


def rot_angle(Ra, Rb):
    import numpy as np
    R = Ra.astype(np.float64) @ Rb.astype(np.float64).T
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arcsin(min(1.0, np.linalg.norm(w))))


def pin_to_gpu_numa_node(local_rank):
    """Host thread on the cores of the GPU's NUMA node (8 ranks fed by one host: keep each rank's launches local).  Best effort."""
    try:
        import torch
        p = torch.cuda.get_device_properties(local_rank)
        bdf = f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}.0"
        node = int(open(f"/sys/bus/pci/devices/{bdf}/numa_node").read())
        if node < 0:
            return None
        cpus = set()
        for part in open(f"/sys/devices/system/node/node{node}/cpulist").read().strip().split(","):
            lo, _, hi = part.partition("-")
            cpus.update(range(int(lo), int(hi or lo) + 1))
        cpus &= os.sched_getaffinity(0)
        if cpus:
            os.sched_setaffinity(0, cpus)
            return node
    except Exception:
        pass
    return None


def shifted(T, d, sign):
    """pose of a scan in a map translated by -d: translate(sign * d) * T"""
    import numpy as np
    out = np.array(T, dtype=np.float32, copy=True)
    out[:3, 3] += sign * np.asarray(d, np.float32)
    return out


def quat_of(R):
    """unit quaternion (x, y, z, w) of a rotation matrix given as nested lists, fp64 (Shepperd's branches).  Plain Python floats: this
    runs on the host between a frame's result and the next frame's first launch, where a numpy call costs more than the arithmetic"""
    import math
    tr = R[0][0] + R[1][1] + R[2][2]
    if tr > 0:
        s = 2.0 * math.sqrt(tr + 1.0)
        q = [(R[2][1] - R[1][2]) / s, (R[0][2] - R[2][0]) / s, (R[1][0] - R[0][1]) / s, 0.25 * s]
    else:
        i = 0 if (R[0][0] >= R[1][1] and R[0][0] >= R[2][2]) else (1 if R[1][1] >= R[2][2] else 2)
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * math.sqrt(1.0 + R[i][i] - R[j][j] - R[k][k])
        q = [0.0, 0.0, 0.0, (R[k][j] - R[j][k]) / s]
        q[i] = 0.25 * s
        q[j] = (R[j][i] + R[i][j]) / s
        q[k] = (R[k][i] + R[i][k]) / s
    nrm = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [q[0] / nrm, q[1] / nrm, q[2] / nrm, q[3] / nrm]


def world_to_body(Tw):
    """(q, t) of the transform that re-expresses world-frame points in the body frame of pose Tw (RGC_odometer.cpp:1250-1255)"""
    M = Tw.tolist() if hasattr(Tw, "tolist") else Tw
    Rt = [[M[0][0], M[1][0], M[2][0]], [M[0][1], M[1][1], M[2][1]], [M[0][2], M[1][2], M[2][2]]]
    tx, ty, tz = M[0][3], M[1][3], M[2][3]
    return quat_of(Rt), [-(Rt[0][0] * tx + Rt[0][1] * ty + Rt[0][2] * tz), -(Rt[1][0] * tx + Rt[1][1] * ty + Rt[1][2] * tz),
                        -(Rt[2][0] * tx + Rt[2][1] * ty + Rt[2][2] * tz)]


def compose_world(Tw, T):
    """world_T * T in fp64 with every entry summed in ascending k -- rgc_align_end_reframe's composition (RGC_odometer.cpp:1201-1203 on
    matrices), so that the last frame of a sequence, which has no next target to enqueue, ends on the same bits as the others (a BLAS
    matmul sums in another order)."""
    import numpy as np
    W = np.zeros((4, 4))
    for a in range(4):
        for b in range(4):
            acc = 0.0
            for k in range(4):
                acc += float(Tw[a, k]) * float(T[k, b])
            W[a, b] = acc
    return W


def make_scans(world, poses, n_source, seeds):
    """synth.make_scan_n(world, poses[i], n_source, seed=seeds[i])["xyz"] for every i, cast on up to 16 host threads (numpy releases the
    interpreter lock in the ray casting; every scan has a generator of its own) -- the arrays one thread would cast, bit for bit."""
    import rgc_slam_amd.synth as synth
    from concurrent.futures import ThreadPoolExecutor
    n_threads = max(1, min(16 // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1"))), len(os.sched_getaffinity(0)), len(poses)))
    with ThreadPoolExecutor(n_threads) as ex:
        return list(ex.map(lambda ps: synth.make_scan_n(world, ps[0], n_source, seed=ps[1])["xyz"], zip(poses, seeds)))


def scan_schedule(n_frames, pool):
    """Which of `pool` distinct scans frame i of an n_frames sequence registers: 0, 1, ..., n_frames - 1 while n_frames <= pool; beyond that
    the trajectory's first `pool` poses forth and back (0 .. pool - 1, pool - 2 .. 0, 1 ..), so that the setup is bounded whatever the number
    of steps and the vehicle never leaves the synthetic world."""
    if n_frames <= pool:
        return list(range(n_frames))
    period = 2 * (pool - 1)
    return [i % period if i % period < pool else period - i % period for i in range(n_frames)]


def make_sequence(synth, world, n_frames, n_source, seed):
    """(poses, scans) of an n_frames dependent sequence: poses[0] the start, scans[i] taken at poses[i + 1] (seed + 100 + its pool index).
    At most SCAN_POOL distinct scans (scan_schedule): entries of a longer sequence repeat the same arrays."""
    pool = min(n_frames, SCAN_POOL)
    poses_pool = synth.make_trajectory(pool + 1, seed=seed)
    scans_pool = make_scans(world, poses_pool[1:], n_source, [seed + 100 + i for i in range(pool)])
    sched = scan_schedule(n_frames, pool)
    return [poses_pool[0]] + [poses_pool[j + 1] for j in sched], [scans_pool[j] for j in sched]


class DependentSequence:
    """The odometer's frame loop on device-resident clouds (RGC_odometer.cpp:976-1023, 1201-1203, 1248-1256):
    frame i: target = the local map re-expressed in the body frame of world pose i - 1 and rebuilt in full (rgc_set_target_reframed,
    on the device), source = scan i, guess = frame i - 1's motion (or a prior), result = the motion of frame i; the world
    pose accumulates in fp64.  overlap: two contexts -- the next scan's preparation (it depends on no pose) is enqueued under the solve."""

    def __init__(self, contexts, d_map, n_map, d_scans, n_scans, pinned=None, d_aligned=None):
        self.v = contexts
        self.d_map, self.n_map, self.d_scans, self.n_scans, self.pinned, self.d_aligned = d_map, n_map, d_scans, n_scans, pinned, d_aligned
        self.d_body = {id(w): w.device_alloc(16 * n_map) for w in contexts}
        self.fitness = self.iterations = None   # (per frame of the last run_cpp)

    def close(self):
        for w in self.v:
            w.device_free(self.d_body[id(w)])

    def frame_target(self, w, Tw_prev):
        q, t = world_to_body(Tw_prev)
        w.setInputTargetReframed(self.d_map, self.n_map, 16, q, t, self.d_body[id(w)])   # B9 + a full per-frame rebuild, like the reference

    def frame_source(self, i, w, from_host=False):
        if from_host:
            w.setInputSource(self.pinned[i].numpy())                                   # H2D inside the step (pinned host memory)
        else:
            w.setInputSourceDevice(self.d_scans[i], self.n_scans[i], 16)

    def run_cpp(self, first, count, Tw0, g0, overlap, stamps=None):
        """run() with the frame loop in C++ (librgc_seq.so: rgc_seq_run_dependent, the calls of rgc::DependentSequence in the same order) --
        the reference's host language, no interpreter between a frame's result and the next frame's first launch.  Scans from the device,
        guess = the previous motion.  Same return value as run().  Falls back to run() when the frame-loop library is not available."""
        import ctypes as C
        import numpy as np
        from rgc_slam_amd import _lib
        S = _lib.load_seq()
        if S is None:
            return self.run(first, count, Tw0, g0, overlap, stamps=stamps)
        a = self.v[0]
        b = self.v[1] if (overlap and len(self.v) > 1) else None
        Tw = np.array(Tw0, dtype=np.float64, order="C")
        g0 = np.ascontiguousarray(g0, np.float32)
        ptrs = (C.c_void_p * count)(*[int(self.d_scans[first + j]) for j in range(count)])
        ns = (C.c_int * count)(*[int(self.n_scans[first + j]) for j in range(count)])
        mot = np.empty((count, 4, 4), np.float32)
        wor = np.empty((count, 4, 4), np.float64)
        st = np.empty(count, np.float64)
        self.fitness, self.iterations = np.empty(count, np.float64), np.empty(count, np.int32)   # (each frame's getFitnessScore and nr_iterations)
        fp, dp, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
        t_call = time.perf_counter()
        rc = S.rgc_seq_run_dependent(a._h, b._h if b is not None else None, C.c_void_p(self.d_map), int(self.n_map), 16, C.c_void_p(self.d_body[id(a)]),
                                     C.c_void_p(self.d_body[id(b)]) if b is not None else None, ptrs, ns, 16, count, Tw.ctypes.data_as(dp),
                                     g0.ctypes.data_as(fp), 1, mot.ctypes.data_as(fp), wor.ctypes.data_as(dp), self.fitness.ctypes.data_as(dp),
                                     self.iterations.ctypes.data_as(ip), st.ctypes.data_as(dp))
        if rc != 0:
            raise RuntimeError(f"rgc_seq_run_dependent: status {rc}: {a._L.rgc_last_error(a._h).decode()} / "
                               f"{b._L.rgc_last_error(b._h).decode() if b is not None else ''}")
        if stamps is not None:
            stamps.extend((t_call + st).tolist())
        motions = [mot[j].copy() for j in range(count)]
        return motions, [wor[j].copy() for j in range(count)], [g0.reshape(4, 4)] + motions[:-1]

    def run(self, first, count, Tw0, g0, overlap, from_host=False, on_result=None, prior_world=None, stamps=None, edit_map=None):
        """frames first .. first + count - 1.  Tw0: world pose before frame `first` (4x4 fp64), g0: its guess (relative, 4x4 fp32).
        prior_world[i]: a world-frame guess of frame i (an IMU-like prior) instead of the previous motion.
        edit_map(i, w): writes what frame i's map differs by into the world-frame map (rgc_upload on w's stream); called for frame i + 1 right
        before frame i's solve is enqueued on w -- behind frame i's map preparation (which has read the map) and in front of its solve
        (whose result the host waits for before it enqueues frame i + 1's preparation): ordered against both without a synchronisation.
        Returns (motions [fp32 4x4], world poses [fp64 4x4], guesses used)."""
        import numpy as np
        v = self.v if overlap else self.v[:1]
        D = len(v)
        Tw, g = np.array(Tw0, dtype=np.float64, order="C"), np.asarray(g0, np.float32)
        motions, worlds, guesses = [], [], []
        if overlap:
            self.frame_source(first, v[0], from_host)
        if edit_map is not None:
            edit_map(first, v[0])
        self.frame_target(v[0], Tw)                   # the first frame's target; every later one is enqueued by align_end_reframe below
        for j in range(count):
            cur, nxt = v[j % D], v[(j + 1) % D]
            if prior_world is not None:
                g = (np.linalg.inv(Tw) @ np.asarray(prior_world[first + j], np.float64)).astype(np.float32)
            if not overlap:
                self.frame_source(first + j, cur, from_host)
            if edit_map is not None and j + 1 < count:
                edit_map(first + j + 1, cur)
            cur.align_begin(g, True)
            if overlap and j + 1 < count:
                nxt.holdSourceUntilTargetOf(cur)                              # ... held back until this frame's map is ready:
                self.frame_source(first + j + 1, nxt, from_host)              # the next scan is prepared under this frame's SOLVE
            if j + 1 < count:
                # the result, the world pose (Tw <- Tw * T, fp64) and the NEXT frame's target -- the map re-expressed in the new body frame,
                # rebuilt in full like the reference does -- in one call: the host's turn-around is on the sequence's critical path
                T = cur.align_end_reframe(nxt, Tw, self.d_map, self.n_map, 16, self.d_body[id(nxt)])
            else:
                T = cur.align_end()
                Tw[:] = compose_world(Tw, T)
            if from_host and self.d_aligned is not None:
                cur.alignedToDevice(self.d_aligned[id(cur)], 16)              # pcl::transformPointCloud(*input_, output, final), left on the device
            if on_result is not None:
                on_result(first + j, cur)
            if stamps is not None:
                stamps.append(time.perf_counter())      # (when this frame's result was in the host's hands)
            guesses.append(g)
            g = T
            motions.append(T)
            worlds.append(Tw.copy())
        return motions, worlds, guesses


def sequences_per_gpu(np, device_index, datasets, frames, reps=6, s_list=(1, 2, 4, 8), reuse=REUSE_NONE):
    """An extra key: S independent dependent sequences on ONE GPU, each on its own pair of contexts and its own C++ host thread
    (rgc-slam_amd/cpp/sequences_per_gpu.cpp over rgc::DependentSequence; compiled here with g++ against the in-tree library and run as a
    child process).  datasets: [(map xyz, pose0, [scan xyz ...]), ...]; sequence s runs dataset s % len(datasets) on its own device copies.
    Every sequence's motions must be those of its run alone, bit for bit."""
    import shutil
    import tempfile
    t0 = time.time()
    tmp = tempfile.mkdtemp(prefix="rgc_seqs_")
    try:
        exe = os.path.join(tmp, "sequences_per_gpu")
        libdir = os.path.join(ROOT, "rgc-slam_amd")
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-pthread", os.path.join(libdir, "cpp", "sequences_per_gpu.cpp"), "-o", exe,
                               "-L", libdir, "-lrgc_hip", "-Wl,-rpath," + libdir])
        def dump(a, path):
            a = np.ascontiguousarray(a, dtype=np.float32)
            with open(path, "wb") as f:
                f.write(np.int32(len(a)).tobytes())
                f.write(a.tobytes())
        dirs = []
        for k, (tgt, pose0, scans) in enumerate(datasets):
            d = os.path.join(tmp, f"d{k}")
            os.makedirs(d)
            dump(tgt, os.path.join(d, "map.bin"))
            with open(os.path.join(d, "pose0.bin"), "wb") as f:
                f.write(np.ascontiguousarray(pose0, np.float64).tobytes())
            for i in range(frames):
                dump(scans[i], os.path.join(d, f"s{i}.bin"))
            dirs.append(d)
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        p = subprocess.run([exe, str(device_index), str(frames), str(reps), str(reuse), ",".join(str(x) for x in s_list), str(len(dirs))] + dirs,
                           capture_output=True, text=True, timeout=900, env=env)
        lines = [l for l in p.stdout.splitlines() if l.strip().startswith("{")]
        if p.returncode != 0 or not lines:
            return {"error": (p.stdout[-300:] + p.stderr[-300:])}
        r = json.loads(lines[-1])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    solo = next((x["aggregate_scans_per_s"] for x in r.get("runs", []) if x["S"] == 1), None)
    for x in r.get("runs", []):
        x["over_one_sequence"] = round(x["aggregate_scans_per_s"] / solo, 3) if solo else None
    r["wall_s_incl_files"] = round(time.time() - t0, 1)
    r["what"] = ("S independent dependent sequences (the c-main workload: full rebuild per frame, nothing kept between frames, like `value`) on ONE GPU, each "
                 "on its own two contexts and its own C++ host thread (no interpreter lock); aggregate = S x passes x frames / wall time of the slowest; "
                 f"{len(datasets)} different synthetic worlds, sequence s runs world s % {len(datasets)} on its own device copies; `value` stays one "
                 "sequence per GPU (north_star)")
    return r


def two_sequences_per_gpu(registration, synth, np, device_index, seq_a, pv_a, n_target, n_source, seed, W, K2, Tw_init, I4, second=None):
    """An extra key: TWO independent dependent sequences on one GPU, each on its own pair of contexts and its own host thread -- what a
    node with more bags than GPUs would do (BASELINE config 4 with fewer than 8 GPUs).  A dependent frame leaves the chip mostly idle
    while it solves (a chain of short launches on 118 workgroups); the other sequence's map preparation fits there.  `value` stays one
    sequence per GPU (north_star).  Each sequence's motions must be those of its solo run, bit for bit."""
    import threading
    t0 = time.time()
    tgt_b, poses_b, scans_b = second
    pv_b = registration.PipelinedVGICP(device_index, depth=2)
    vb = pv_b.v[0]
    for w in pv_b.v:
        w.setNeighbourReuse(REUSE_NONE)   # like `value`: nothing kept from one frame's target to the next
    def to_dev(xyz):
        a = np.zeros((xyz.shape[0], 4), np.float32)
        a[:, :3] = xyz
        p = vb.device_alloc(a.nbytes)
        vb.upload(p, a)
        return p
    d_map_b, d_scans_b = to_dev(tgt_b), [to_dev(s_) for s_ in scans_b]
    seq_b = DependentSequence(pv_b.v, d_map_b, tgt_b.shape[0], d_scans_b, [s_.shape[0] for s_ in scans_b])
    for w in pv_b.v:   # context start-up, as for the first sequence
        seq_b.v = [w]
        seq_b.run(0, 1, np.asarray(poses_b[0], np.float64), I4, False)
    seq_b.v = pv_b.v
    starts = {}
    for name, sq, p0 in (("a", seq_a, Tw_init), ("b", seq_b, np.asarray(poses_b[0], np.float64))):
        Tw_s, g_s = p0, I4
        if W > 0:
            m, wd, _ = sq.run(0, W, p0, I4, True)
            Tw_s, g_s = wd[-1], m[-1]
        starts[name] = (Tw_s, g_s)
    REPS = 6
    def solo(sq, name):
        per, ref = [], None
        for r in range(REPS):
            for w in sq.v:
                w.synchronize()
            tr = time.perf_counter()
            m, _, _ = sq.run(W, K2, starts[name][0], starts[name][1], True)
            for w in sq.v:
                w.synchronize()
            per.append(time.perf_counter() - tr)
            ref = m if ref is None else ref
        return ref, float(np.median(per[1:]))
    ref_a, t_a = solo(seq_a, "a")
    ref_b, t_b = solo(seq_b, "b")
    # together: both threads leave a barrier at once and run their K2 frames REPS times; the job is done when the slower one is
    gate = threading.Barrier(3)
    same = {"a": True, "b": True}
    switch0 = sys.getswitchinterval()
    sys.setswitchinterval(2.0e-5)   # two Python threads drive the two sequences: the interpreter lock changes hands at this interval (default 5 ms) when both want it
    def worker(sq, name, ref):
        gate.wait()
        for r in range(REPS):
            m, _, _ = sq.run(W, K2, starts[name][0], starts[name][1], True)
            same[name] = same[name] and all(np.array_equal(x, y) for x, y in zip(ref, m))
        for w in sq.v:
            w.synchronize()
    th = [threading.Thread(target=worker, args=(seq_a, "a", ref_a)), threading.Thread(target=worker, args=(seq_b, "b", ref_b))]
    for t_ in th:
        t_.start()
    gate.wait()
    tr = time.perf_counter()
    for t_ in th:
        t_.join()
    wall = time.perf_counter() - tr
    sys.setswitchinterval(switch0)
    seq_b.close()
    for p in [d_map_b] + d_scans_b:
        vb.device_free(p)
    pv_b.close()
    return {"aggregate_scans_per_s": round(2 * K2 * REPS / wall, 3), "ms_per_step_per_sequence": round(1e3 * wall / (K2 * REPS), 4),
            "solo_scans_per_s": [round(K2 / t_a, 3), round(K2 / t_b, 3)], "frames_per_sequence": K2 * REPS,
            "same_poses_as_each_sequence_alone": bool(same["a"] and same["b"]), "seeds": [int(seed), int(seed + 1)],
            "wall_s_incl_datagen": round(time.time() - t0, 1),
            "what": "two independent dependent sequences (two maps, two trajectories) on ONE GPU, each on its own two contexts and host thread, "
                    "full rebuild per frame with nothing kept between frames (RGC_REUSE_NONE, like `value`); aggregate = frames of both / wall time of the "
                    "slower; driven by two PYTHON threads (the interpreter lock is part of the figure: sequences_per_gpu is the C++ measurement)"}


def roofline_by_kernel(n_s, n_t, n_vox, n_corr, t_cells, s_cells, deferred_src, frame_traffic):
    """The five kernels with the most GPU time per frame of the timed workload (profiles/KERNEL_STATS_FILE: rocprofv3 --kernel-trace over the
    dependent c-main sequence on two contexts, RGC_REUSE_NONE), each with its algorithmic bytes per frame / its GPU time per frame / 8 TB/s
    and the measured HBM bytes of the same kernel (profiles/FRAME_TRAFFIC_FILE).  Algorithmic bytes: SURVEY 8d's terms for the kernels 8d
    covers; for the grid build (8d has no term: the reference's kd-tree build is not in B) the bytes the pass cannot avoid -- its input
    once, its output once."""
    kt, kt_src = profile_json(KERNEL_STATS_FILE)
    if not kt or not kt.get("per_kernel"):
        return None
    both = n_t + n_s
    alg = [  # (name prefix, bytes per FRAME, what)
        ("k_knn_sp<20, true", 36.0 * n_t, "8d: 12 B read + 24 B written per map point"),
        ("k_knn_sp<20, false", 36.0 * (n_s - deferred_src), "8d: 36 B per scan point it resolves itself"),
        ("k_knn_coop<20, false", 36.0 * deferred_src, "8d: 36 B per deferred scan point"),
        ("k_voxel_build_coop", 36.0 * n_t + 40.0 * n_vox, "8d: 36 B per map point + 40 B per voxel"),
        ("k_lm_step", None, "8d: 36 B per scan point + 40 B per correspondence, per launch"),
        ("k_count<true>", 40.0 * n_t, "own: 16 B read + 16 B re-framed point written + 8 B cell / slot per map point"),
        ("k_count<false>", 24.0 * n_s, "own: 16 B read + 8 B cell / slot per scan point"),
        ("k_place", 16.0 * both, "own: 8 B read + 8 B record written per point (both clouds)"),
        ("k_rank_gather", 40.0 * both, "own: 8 B record + 16 B point read, 16 B sorted point written (both clouds)"),
        ("k_cells_reduce", 4.0 * (t_cells + s_cells), "own: one counter per grid cell read (both clouds)"),
        ("k_cells_scan_write", 12.0 * t_cells + 8.0 * s_cells, "own: counter read, start (+ voxel id for the map) written per cell"),
        ("k_voxel_patch", None, None), ("k_fitness", 24.0 * n_s, "own: 12 B per scan point read, 1-NN"),
    ]
    traffic = {}
    if frame_traffic:
        for r in frame_traffic.get("per_kernel", []):
            traffic[r["kernel"]] = r
    rows = []
    for r in sorted(kt["per_kernel"], key=lambda x: -x["us_per_frame"])[:5]:
        name = r["kernel"]
        b, what = None, None
        for pre, bytes_, w in alg:
            if name.startswith(pre):
                b, what = bytes_, w
                if pre == "k_lm_step":
                    b = r["launches_per_frame"] * (36.0 * n_s + 40.0 * n_corr)
                break
        row = {"kernel": name, "us_per_frame": r["us_per_frame"], "launches_per_frame": r["launches_per_frame"], "avg_launch_us": r["avg_us"],
               "algorithmic_bytes_per_frame": None if b is None else round(b), "algorithmic_bytes": what}
        if b is not None and r["us_per_frame"] > 0:
            row["achieved_GBps"] = round(b / (r["us_per_frame"] * 1e-6) / 1e9, 2)
            row["frac_of_hbm_peak"] = round(b / (r["us_per_frame"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 5)
        t = next((v_ for k_, v_ in traffic.items() if name.startswith(k_) or k_.startswith(name)), None)
        if t:
            row["measured_MB_per_frame"] = t["MB_per_frame"]
            if b:
                row["measured_over_algorithmic"] = round(t["MB_per_frame"] * 1e6 / b, 2)
        rows.append(row)
    return {"kernels": rows, "gpu_time_source": kt_src, "traffic_source": frame_traffic and "profiles/" + FRAME_TRAFFIC_FILE,
            "kernel_us_per_frame_total": kt.get("kernel_us_per_frame_total"), "workload": kt.get("workload")}


def frame_bytes(st, n_s, n_t):
    """SURVEY §8d's yardstick from one frame's counters"""
    return algorithmic_bytes(n_s, n_t, st["n_voxels"], st["n_corr"], st["n_linearize"], st["n_error"])


def time_config(registration, oracle, name, tgt, scans, pose0, prior=None, dependent=True):
    """scans[i] registered to tgt; frame 0 is the warm-up (once per context); frame 1 is checked against the CPU oracle.
    dependent: the target of frame i is tgt re-expressed in the body frame of pose i - 1 (DependentSequence); else tgt is a FIXED map
    in its own frame (c1, the reference's CPU-runnable case) and a frame's whole preparation may overlap the previous solve.
    Timed twice: two contexts (the figure) and one frame at a time."""
    import numpy as np
    pv = registration.PipelinedVGICP(int(os.environ.get("LOCAL_RANK", "0")), depth=2)
    v = pv.v[0]
    for w in pv.v:
        w.setNeighbourReuse(REUSE_NONE)   # like `value`: every frame's target is searched in full

    def to_dev(xyz):
        a = np.zeros((xyz.shape[0], 4), np.float32)
        a[:, :3] = xyz
        p = v.device_alloc(a.nbytes)
        v.upload(p, a)
        return p
    d_tgt, d_s = to_dev(tgt), [to_dev(s) for s in scans]
    frames = len(scans) - 1
    I4 = np.eye(4, dtype=np.float32)
    if dependent:
        seq = DependentSequence(pv.v, d_tgt, len(tgt), d_s, [len(s) for s in scans])
        Tw0 = np.asarray(pose0, np.float64)
        for k, w in enumerate(pv.v):   # context start-up: frame 0 once on each
            seq.v = [w]
            _, w0, _ = seq.run(0, 1, Tw0, I4, False, prior_world=prior)
        seq.v = pv.v
        Tw1 = w0[0]
        pv.synchronize()
        gc.collect()
        gc.freeze()
        # (the few timed frames are run REPS times over from the same start -- the same frames, the same poses -- and the median pass counts:
        # a three-frame pass is at the mercy of one hiccup)
        REPS, same_reps = 5, True
        def timed(overlap):
            nonlocal same_reps
            els, first = [], None
            for _ in range(REPS):
                t1 = time.perf_counter()
                m, _, gq = seq.run(1, frames, Tw1, I4, overlap, prior_world=prior)
                pv.synchronize()
                els.append(time.perf_counter() - t1)
                if first is None:
                    first = (m, gq)
                else:
                    same_reps = same_reps and all(np.array_equal(x, y) for x, y in zip(first[0], m))
            return float(np.median(els)), first[0], first[1]
        el_seq, m_seq, g_seq = timed(False)
        el, m_pipe, _ = timed(True)
        fin, fin_seq, g_in1 = m_pipe, m_seq, g_seq[0]
        st = pv.v[(frames - 1) % 2].stats()
        # the same frames with the lazy target (covariances and voxels only where the solve can look; bench.py's `lazy_target` key)
        for w in pv.v:
            w.setLazyTarget(2)
        seq.run(1, frames, Tw1, I4, True, prior_world=prior)   # (once untimed: the stamp array's allocation)
        pv.synchronize()
        el_lazy, m_lazy, _ = timed(True)
        lazy_info = {"lazy_target_scans_per_s": round(frames / el_lazy, 2), "lazy_target_same_poses": bool(same_reps and all(np.array_equal(x, y) for x, y in zip(m_pipe, m_lazy))),
                     "timed_passes": REPS,
                     "lazy_target_solves_repeated": int(sum(w.stats()["lazy_misses"] for w in pv.v))}
        for w in pv.v:
            w.setLazyTarget(0)
        # ... and with the library's default (seeds + neighbour lists of a map it verifies unchanged): this synthetic map never changes
        for w in pv.v:
            w.setNeighbourReuse(REUSE_LISTS)
        seq.run(1, frames, Tw1, I4, True, prior_world=prior)   # (once untimed: the first search builds the lists)
        pv.synchronize()
        el_reuse, m_reuse, _ = timed(True)
        lazy_info["reuse_unchanged_map_scans_per_s"] = round(frames / el_reuse, 2)
        lazy_info["reuse_unchanged_map_same_poses"] = bool(same_reps and all(np.array_equal(x, y) for x, y in zip(m_pipe, m_reuse)))
        for w in pv.v:
            w.setNeighbourReuse(REUSE_NONE)
    else:
        def setc(i, w):
            w.setInputTargetDevice(d_tgt, len(tgt), 16)
            w.setInputSourceDevice(d_s[i], len(scans[i]), 16)
        guess0 = np.asarray(pose0, np.float32)
        for w in pv.v:
            setc(0, w)
            w.align(guess0, want_output=False, want_fitness=True)
        g_in1 = v.getFinalTransformation()
        pv.synchronize()
        # a cyclic-GC pass over torch's object graph (40-65 ms, scripts/exp_stall.py) inside a 3-frame timed region quarters the figure:
        # the garbage made so far (data generation, the oracle's arrays) is collected here and the survivors are frozen, as before the main loop
        gc.collect()
        gc.freeze()
        t1 = time.perf_counter()
        g, fin_seq = g_in1, []
        for i in range(1, frames + 1):
            setc(i, v)
            v.align(g, want_output=False, want_fitness=True)
            g = v.getFinalTransformation()
            fin_seq.append(g)
        v.synchronize()
        el_seq = time.perf_counter() - t1
        t1 = time.perf_counter()
        fin = pv.run(frames, lambda j, w: setc(j + 1, w), g_in1, want_fitness=True)
        pv.synchronize()
        el = time.perf_counter() - t1
        st = pv.v[(frames - 1) % 2].stats()
        lazy_info = {}
    B = frame_bytes(st, len(scans[0]), len(tgt))
    out = {"config": name, "n_source": int(len(scans[0])), "n_target": int(len(tgt)), "frames": frames,
           "sequence": "dependent (target re-framed by the previous pose)" if dependent else "fixed map",
           "scans_per_s": round(frames / el, 2), "ms_per_scan": round(1e3 * el / frames, 3),
           "one_frame_at_a_time_scans_per_s": round(frames / el_seq, 2),
           "same_poses_both_ways": bool(all(np.array_equal(x, y) for x, y in zip(fin, fin_seq))), "outer_iterations_last": st["outer_iterations"],
           "algorithmic_bytes_per_scan": round(B), "hbm_frac_whole_frame": round(B * frames / el / 1e9 / HBM_PEAK_GBS, 6)}
    out.update(lazy_info)
    if oracle is not None:
        o = oracle.Registration(num_threads=min(14, os.cpu_count() or 1))  # the reference's setNumThreads(14): also the oracle's faster setting
        if dependent:   # identical input clouds: the target the GPU path registered frame 1 to
            q, t = world_to_body(Tw1)
            v.transformCloudDevice(d_tgt, len(tgt), 16, q, t, seq.d_body[id(v)])
            tgt1 = v.download(seq.d_body[id(v)], (len(tgt), 4))[:, :3].copy()
        else:
            tgt1 = tgt
        c0 = time.perf_counter()
        o.set_target(tgt1)
        o.set_source(scans[1])
        To = o.align(g_in1)
        _ = o.fitness()
        out["cpu_oracle_scans_per_s"] = round(1.0 / (time.perf_counter() - c0), 4)
        out["max_dt_m"] = float(np.abs(fin[0][:3, 3] - To[:3, 3]).max())
        out["max_dtheta_rad"] = rot_angle(fin[0][:3, :3], To[:3, :3])
    pv.close()
    return out


def run_extra_configs(registration, synth, oracle, keys):
    """BASELINE.json's other single-GPU configurations, a few frames each (scripts/bench_configs.py runs them at length):
    c1 30 k vs a FIXED 100 k map; c3 HDL-64 130 k vs a 5 M rolling map; c5 two interleaved 64-beam patterns 250 k vs 20 M (four copies of
    the 5 M tile) with the true pose corrupted by ~0.5 deg of rotation as the IMU-like prior.  c3 and c5 are dependent sequences."""
    import numpy as np
    res = []
    def guarded(name, fn):
        try:
            t0 = time.time()
            r = fn()
            r["wall_s_incl_datagen"] = round(time.time() - t0, 1)
            res.append(r)
        except Exception as e:  # the metric line must not be lost to a side configuration
            res.append({"config": name, "error": str(e)[:200]})
    if "c1" in keys:
        def c1():
            world, tgt = synth.make_world_and_map(100000, seed=synth.SEED)
            poses = synth.make_trajectory(12, seed=synth.SEED)
            scans = [synth.make_scan_n(world, poses[i + 1], 30000, seed=synth.SEED + 100 + i)["xyz"] for i in range(11)]
            return time_config(registration, oracle, "c1: VLP-16 30 k-pt scans vs 100 k-pt fixed map", tgt, scans, poses[0], dependent=False)
        guarded("c1", c1)
    if "c3" in keys or "c5" in keys:
        world = tile = None
        try:
            world, tile = synth.make_world_and_map(5_000_000, seed=synth.SEED + 7)
        except Exception as e:
            res.append({"config": "c3/c5", "error": str(e)[:200]})
        e64 = synth.hdl64_elev()
        if tile is not None and "c3" in keys:
            def c3():
                poses = synth.make_trajectory(8, seed=synth.SEED + 7)
                scans = [synth.make_scan_n(world, poses[i + 1], 130000, elev_deg=e64, seed=synth.SEED + 200 + i)["xyz"] for i in range(6)]
                return time_config(registration, oracle, "c3: HDL-64 130 k-pt scans vs 5 M-pt rolling map", tile, scans, poses[0])
            guarded("c3", c3)
        if tile is not None and "c5" in keys:
            def c5():
                L = 2.0 * world.half_extent + 4.0
                tgt = np.concatenate([tile, tile + np.float32([L, 0, 0]), tile + np.float32([0, L, 0]), tile + np.float32([L, L, 0])]).astype(np.float32)
                poses = synth.make_trajectory(6, seed=synth.SEED + 9)
                from rgc_slam_amd import odometry
                # the guesses the odometer forms with USE_IMU = 1 (RGC_odometer.cpp:929-931, 993-996): the gyro's pre-integrated rotation over
                # the sweep (synthetic 200 Hz IMU stream through rgc_imu_preintegrate) and the previous sweep's translation
                imu_prior = odometry.imu_rotation_priors(poses)
                scans, prior = [], {}
                for i in range(4):
                    a = synth.make_scan_n(world, poses[i + 1], 125000, elev_deg=e64, seed=synth.SEED + 300 + i)["xyz"]
                    b = synth.make_scan_n(world, poses[i + 1], 125000, elev_deg=e64 + 0.5 * float(np.abs(np.diff(np.sort(e64))).min()),
                                          seed=synth.SEED + 400 + i)["xyz"]
                    scans.append(np.concatenate([a, b]).astype(np.float32))
                    prior[i] = imu_prior[i + 1]
                return time_config(registration, oracle, "c5: 2 x 64-beam 250 k-pt scans vs 20 M-pt rolling map, IMU-preintegrated prior", tgt, scans,
                                   poses[0], prior=prior)
            guarded("c5", c5)
    return res


def pose_checksums(np, worlds, world_size, dist):
    """(this rank's checksum of its world poses, every rank's): one small object per rank, for the record that the ranks ran DIFFERENT sequences"""
    checksum = float(np.sum(np.abs(np.asarray(worlds, np.float64))))
    rank_checksums = [checksum]
    if world_size > 1:
        rank_checksums = [None] * world_size
        dist.all_gather_object(rank_checksums, checksum)
    return checksum, rank_checksums


def dump_outputs(out_dir, suffix, np, motion, world, fitness, iterations):
    """What a caller of the timed path receives for its last step: the motion (fp32 4x4), the world pose (fp64 4x4), getFitnessScore and
    nr_iterations (fp64), as <out_dir>/<name><suffix>.npy"""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"motion": np.asarray(motion, np.float32), "world_pose": np.asarray(world, np.float64)}
    if fitness is not None:
        arrays["fitness"] = np.asarray(fitness[-1:], np.float64)
        arrays["iterations"] = np.asarray(iterations[-1:], np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + suffix + ".npy"), a)


def headline(args, K, W, world_size, elapsed, step_stamps, prewarm, searched, host_loop, checksum, rank_checksums, np):
    """The keys of every result line: the metric and what it was measured on"""
    return {
        "metric": "registered scans/sec (16-beam -> 1M-pt map)", "value": round(K * world_size / elapsed, 3), "unit": "scans/s",
        "n_gpus": world_size, "steps": K, "warmup": W, "prewarm_frames_before_the_warmup": 4 * prewarm, "ms_per_step": round(1e3 * elapsed / K, 3),
        "timed_steps_ms": {"median": round(1e3 * float(np.median(np.diff(step_stamps))), 4), "max": round(1e3 * float(np.max(np.diff(step_stamps))), 4),
                           "slowest_step": int(np.argmax(np.diff(step_stamps))),
                           "what": "host time between consecutive results inside the timed region of rank 0 (a one-off stall -- an allocation, a speculative-grid miss -- shows here, not in the kernels)"},
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32 points and neighbour search, f64 covariances and solve",
        "data": "synthetic",
        "config": {"workload": f"c-main: a dependent sequence of synthetic VLP-16 {args.n_source}-pt scans, each registered to the {args.n_target}-pt local "
                               f"map re-expressed in the previous pose's body frame on the device and rebuilt in full, nothing kept from one "
                               f"frame's target to the next (rgc_set_knn_reuse(RGC_REUSE_NONE): all {args.n_target} queries searched every frame, as for "
                               f"a map whose point set changes every frame -- the reference's does; BASELINE.md c-main; RGC_odometer.cpp:976-1256; one "
                               f"independent sequence per GPU; only the next scan's preparation overlaps a solve)",
                   "n_source": args.n_source, "n_target": args.n_target, "voxel_res": 1.0, "k": 20, "max_iterations": 25,
                   "knn_reuse": "none", "queries_searched_per_frame": searched, "host_frame_loop": host_loop,
                   "parallelism": f"sequences x{world_size}", "distinct_scans": min(K + W, SCAN_POOL)},
        "final_pose_checksum": checksum,
        "final_pose_checksum_per_rank": rank_checksums,
        "sequence_of_rank0": args.sequence,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=20)   # (a few milliseconds of the same steps in front of the timed ones: the first steps behind an idle GPU run at lower clocks)
    ap.add_argument("--n-target", type=int, default=N_TARGET)
    ap.add_argument("--n-source", type=int, default=N_SOURCE)
    ap.add_argument("--full", action="store_true", help="after the timed steps, everything else this benchmark measures and checks: the extra keys "
                    "of the module docstring, the CPU baseline and the other configurations; without it the line holds the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the timed path computed in its last step (motion, world pose, fitness, "
                    "iterations) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--configs", default="c1,c3,c5", help="with --full: extra single-GPU configurations of BASELINE.json to run after the metric (c1,c3,c5 or 'none')")
    ap.add_argument("--no-two-sequences", action="store_true", help="with --full: skip the extra key two_sequences_per_gpu (a second sequence's data and contexts)")
    ap.add_argument("--sequence", type=int, default=0, help="number of the first rank's sequence (rank r runs sequence --sequence + r: seed offset)")
    args = ap.parse_args()

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world_size == 1:
        # not launched through torch.distributed.run: start it as a child (nothing here has touched the GPU yet)
        port = 29500 + (os.getpid() % 2000)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    import numpy as np
    import torch  # first: its bundled HIP runtime must be the one librgc_hip.so binds to in this process
    import torch.distributed as dist

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    # RGC_BENCH_DEVICE: every rank on THIS device (tests/test_gpu_bench_contract.py runs two ranks on a one-GPU box: the N > 1 control flow
    # with real HIP contexts in more than one process; RCCL cannot span two ranks of one device, so the barrier / MAX-reduce then go over
    # gloo -- RGC_BENCH_DIST_BACKEND).  Unset (the driver's runs): rank r on device r, RCCL.
    device_index = int(os.environ.get("RGC_BENCH_DEVICE", local_rank))
    backend = os.environ.get("RGC_BENCH_DIST_BACKEND", "nccl")
    torch.cuda.set_device(device_index)
    numa = pin_to_gpu_numa_node(device_index)
    if world_size > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world_size, device_id=torch.device("cuda", device_index))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world_size)

    import rgc_slam_amd.synth as synth
    from rgc_slam_amd import registration

    K, W = args.steps, args.warmup
    seed = synth.SEED + args.sequence + rank  # one independent sequence per rank
    t0 = time.time()
    world, tgt = synth.make_world_and_map(args.n_target, seed=seed)
    poses, scans = make_sequence(synth, world, K + W, args.n_source, seed)
    maps = [(tgt - np.asarray(d, np.float32)).astype(np.float32) for d in (MAP_SHIFTS if args.full else MAP_SHIFTS[:1])]
    log(f"[rank {rank}] synthetic data: map {tgt.shape}, {len(scans)} scans of {scans[0].shape[0]} pts, world half-extent "
        f"{world.half_extent:.1f} m, {time.time() - t0:.1f} s, NUMA node {numa}")

    pv = registration.PipelinedVGICP(device_index, depth=2)
    v = pv.v[0]
    # `value` and every key that is not under `reuse_*`: nothing is carried from one step's target to the next (see the module docstring)
    for w in pv.v:
        w.setNeighbourReuse(REUSE_NONE)
    # inputs resident in HBM (x,y,z,pad; 16-byte stride) before anything is timed
    def to_dev(xyz):
        a = np.zeros((xyz.shape[0], 4), np.float32)
        a[:, :3] = xyz
        p = v.device_alloc(a.nbytes)
        v.upload(p, a)
        return p
    d_maps = [to_dev(m) for m in maps]   # [0] is the map in the world frame; the others only serve `replay_of_preframed_maps`
    d_pool = {}                          # (one device copy of each distinct scan: a sequence longer than SCAN_POOL repeats them)
    for s in scans:
        if id(s) not in d_pool:
            d_pool[id(s)] = to_dev(s)
    d_scans = [d_pool[id(s)] for s in scans]
    pinned = d_aligned = None
    if args.full:
        # scan_h2d_and_output's inputs: every scan in pinned host memory (x,y,z,pad), one device buffer per context for align()'s output cloud
        pinned_pool = {}
        for s in scans:
            if id(s) not in pinned_pool:
                t = torch.zeros((s.shape[0], 4), dtype=torch.float32).pin_memory()
                t[:, :3] = torch.from_numpy(s)
                pinned_pool[id(s)] = t
        pinned = [pinned_pool[id(s)] for s in scans]
        d_aligned = {id(w): w.device_alloc(16 * args.n_source) for w in pv.v}
    seq = DependentSequence(pv.v, d_maps[0], tgt.shape[0], d_scans, [s.shape[0] for s in scans], pinned, d_aligned)
    I4 = np.eye(4, dtype=np.float32)
    Tw_init = np.asarray(poses[0], np.float64)

    per_frame = []
    def collect(i, w):
        st = w.stats()
        per_frame.append((st["outer_iterations"], st["n_linearize"], st["n_error"], st["n_corr"], st["n_voxels"], st["target_cells"], st["source_cells"],
                          st["deferred_source"], st["deferred_target"]))

    for w in pv.v:   # context start-up (first allocations, the first cloud's bounding-box round trip): frame 0 once on each, untimed
        seq.v = [w]
        seq.run(0, 1, Tw_init, I4, False)
    seq.v = pv.v
    # The one-off ~40 ms stall that earlier rounds hid behind 96 untimed frames is CPython's cyclic garbage collector doing a full
    # collection over torch's object graph (scripts/exp_stall.py: gone with gc.freeze(), unmoved by anything done to the HIP
    # runtime): it belongs to this harness, not to the path.  Freeze what exists; the loops below allocate nothing cyclic.
    # (Before the warm-up, so that the timed loop follows it directly: 50 ms of host-only work would let the GPU's clocks drop.)
    gc.collect()
    gc.freeze()
    # HIP-event regions cost two hipEventRecord each: in the timed loop only the dominant kernel (the map's bulk kNN +
    # covariance launch -- rocprofv3 agrees, profiles/) is bracketed; the other stages are timed in a separate pass below.
    DOMINANT = "knn_cov_target"
    for w in pv.v:
        w.profile_enable(True)
        w.profile_select([DOMINANT])
    Tw_start, g_start = Tw_init, I4
    from rgc_slam_amd import _lib as _rgc_lib
    host_loop = "c++ (librgc_seq.so: rgc_seq_run_dependent)" if _rgc_lib.load_seq() is not None else "python (ctypes call per stage)"
    # A device that has been idle (15 s of data generation, the collection above) starts at low clocks and takes a few milliseconds of work to
    # leave them -- longer than the W warm-up steps a caller may ask for last.  The first frames of the sequence, PREWARM times over, untimed, in
    # front of the W warm-up steps: the timed steps then run at the clocks a sequence that keeps running sees (steady_state below).
    PREWARM = 8
    for _ in range(PREWARM):
        seq.run_cpp(0, min(4, K + W), Tw_init, I4, True)
    if W > 0:
        m, wd, _ = seq.run_cpp(0, W, Tw_init, I4, True)
        Tw_start, g_start = wd[-1], m[-1]
    pv.synchronize()
    for w in pv.v:
        w.profile_reset()
    if world_size > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    step_stamps = [t_start]
    motions, worlds, guesses = seq.run_cpp(W, K, Tw_start, g_start, True, stamps=step_stamps)   # (the K steps: one call into the C++ frame loop; per-frame counters are read in an untimed repetition below)
    pv.synchronize()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t_start
    if world_size > 1:
        dist.barrier()
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, "" if rank == 0 else f"_rank{rank}", np, motions[-1], worlds[-1], seq.fitness, seq.iterations)
    if not args.full:
        checksum, rank_checksums = pose_checksums(np, worlds, world_size, dist)
        searched = int(pv.v[(K - 1) % len(pv.v)].stats()["searched_target"]) if K > 0 else 0   # (the target of the last timed frame)
        seq.close()
        pv.close()
        if rank == 0:
            print(json.dumps(headline(args, K, W, world_size, elapsed, step_stamps, PREWARM, searched, host_loop, checksum, rank_checksums, np)), flush=True)
        if world_size > 1:
            dist.destroy_process_group()
        return
    prof_dom = {"total_ms": 0.0, "launches": 0, "points": 0}
    for w in pv.v:
        d = w.profile()[DOMINANT]
        for kk in prof_dom:
            prof_dom[kk] += d[kk]
        w.profile_enable(False)
    # the same K steps one at a time on one context through the blocking calls (what a caller of align() gets: the frame's latency)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    seq_motions, _, _ = seq.run_cpp(W, K, Tw_start, g_start, False)
    v.synchronize()
    elapsed_seq = time.perf_counter() - t1
    seq_same = bool(all(np.array_equal(a_, b_) for a_, b_ in zip(motions, seq_motions)))
    # the same K steps with the scan crossing PCIe inside the step and the output cloud produced (device-resident): an extra key
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    h2d_motions, _, _ = seq.run(W, K, Tw_start, g_start, True, from_host=True)
    pv.synchronize()
    elapsed_h2d = time.perf_counter() - t2
    h2d_same = bool(np.array_equal(h2d_motions[-1], motions[-1]))
    # round 2's figure, named for what it is: targets that do not depend on the previous pose (three translated copies of the map in
    # turn), so a whole frame's preparation runs under the previous frame's solve -- a replay of pre-framed sub-maps, not a live sequence
    def set_clouds(i, w):
        w.setInputTargetDevice(d_maps[i % len(maps)], tgt.shape[0], 16)
        w.setInputSourceDevice(d_scans[i], scans[i].shape[0], 16)
    to_map = lambda i, T_world: shifted(T_world, MAP_SHIFTS[i % len(maps)], -1.0)
    to_world = lambda i, T: shifted(T, MAP_SHIFTS[i % len(maps)], +1.0)
    g_world = np.asarray(Tw_start, np.float32)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    Ts = pv.run(K, lambda j, w: set_clouds(W + j, w), to_map(W, g_world), want_fitness=True,
                next_guess=lambda j, T: to_map(W + j + 1, to_world(W + j, T)))
    pv.synchronize()
    elapsed_replay = time.perf_counter() - t3
    replay_err = float(max(np.abs(to_world(W + j, T).astype(np.float64) - worlds[j]).max() for j, T in enumerate(Ts)))
    # The K timed steps are ~18 ms of GPU work behind a warm-up of W steps, with the dominant kernel bracketed by HIP events (two records per
    # frame: ~3 % of a frame).  The same K steps repeated back to back without the events (an extra key, not `value`): what a sequence
    # that keeps running sustains, and a check that every repetition gives the timed run's poses bit for bit.
    REPS = 10
    steady = {}
    for mode, overlap in (("two_contexts", True), ("one_frame_at_a_time", False)):
        per, same = [], True
        for r in range(REPS):
            pv.synchronize()
            tr = time.perf_counter()
            if r == 0:   # (repetition 0 through the Python loop: the frames' counters; not in the median)
                mr, _, _ = seq.run(W, K, Tw_start, g_start, overlap, on_result=collect if overlap else None)
            else:
                mr, _, _ = seq.run_cpp(W, K, Tw_start, g_start, overlap)
            pv.synchronize()
            per.append(time.perf_counter() - tr)
            same = same and all(np.array_equal(a_, b_) for a_, b_ in zip(motions, mr))
        med = float(np.median(per[2:]))
        steady[mode] = {"scans_per_s": round(K / med, 3), "ms_per_step": round(1e3 * med / K, 4), "same_poses_every_repetition": bool(same)}
    # ... and the same through the Python frame loop (a ctypes call per stage): what the interpreter costs a dependent sequence
    per = []
    for r in range(5):
        pv.synchronize()
        tr = time.perf_counter()
        mr, _, _ = seq.run(W, K, Tw_start, g_start, True)
        pv.synchronize()
        per.append(time.perf_counter() - tr)
    med = float(np.median(per[1:]))
    steady["two_contexts_python_frame_loop"] = {"scans_per_s": round(K / med, 3), "ms_per_step": round(1e3 * med / K, 4),
                                                "same_poses": bool(all(np.array_equal(a_, b_) for a_, b_ in zip(motions, mr)))}
    steady["what"] = (f"the K timed steps repeated {REPS} times back to back with no HIP events in the loop, median of the last {REPS - 2} repetitions: the "
                      f"rate of a sequence that keeps running, beside `value` (first pass behind W warm-up steps, dominant kernel bracketed by events)")
    # Lazy target (an extra key; `value` above stays the full rebuild, like the reference): covariances and voxels only where the solve can
    # look -- the cells within two voxels of where the scan falls at the guess, every look-up checked, a miss repeats the solve on the
    # completed map (rgc_set_target_lazy).  The same K steps, the same poses bit for bit.
    LAZY_MARGIN = 2
    lazy = {}
    for w in pv.v:
        w.setLazyTarget(LAZY_MARGIN)
    miss0 = sum(w.stats()["lazy_misses"] for w in pv.v)
    for mode, overlap in (("two_contexts", True), ("one_frame_at_a_time", False)):
        per, same = [], True
        for r in range(6):
            pv.synchronize()
            tr = time.perf_counter()
            mr, _, _ = seq.run(W, K, Tw_start, g_start, overlap)
            pv.synchronize()
            per.append(time.perf_counter() - tr)
            same = same and all(np.array_equal(a_, b_) for a_, b_ in zip(motions, mr))
        med = float(np.median(per[1:]))
        lazy[mode] = {"scans_per_s": round(K / med, 3), "ms_per_step": round(1e3 * med / K, 4), "same_poses_as_the_full_rebuild": bool(same)}
    lazy["solves_repeated_on_the_completed_map"] = int(sum(w.stats()["lazy_misses"] for w in pv.v) - miss0)
    lazy["margin_cells"] = LAZY_MARGIN
    lazy["what"] = ("rgc_set_target_lazy: the map's grid is built in full, its 20-NN covariances and voxels only within margin_cells voxels of a voxel the "
                    "scan falls into at the guess (fast_vgicp_impl.hpp:73-116: only looked-up voxels enter the cost); the solve checks every look-up and "
                    "repeats on the completed map if one lands outside; medians of 5 repetitions of the K timed steps")
    for w in pv.v:
        w.setLazyTarget(0)
    # the dominant kernel by itself (nothing else on the GPU): what the launch costs, as opposed to what it costs while it shares the chip
    # with the other context's scan preparation -- the launch the timed region runs: the full search of the map re-framed by the timed
    # frames' own poses
    v.profile_enable(True)
    v.profile_select([DOMINANT])
    seq.frame_target(v, Tw_start)
    v.synchronize()
    v.profile_reset()
    for j in range(5):
        seq.frame_target(v, worlds[j % len(worlds)])
        v.synchronize()
    dom_alone = v.profile()[DOMINANT]
    searched_alone = int(v.stats()["searched_target"])
    v.profile_enable(False)
    # per-stage breakdown: a few more frames, one at a time, with every region bracketed (untimed, informational)
    v.profile_enable(True)
    v.profile_select(None)
    v.profile_reset()
    KB = min(K, 5)
    seq.run(W, KB, Tw_start, g_start, False)   # the same frames with the same guesses as the timed loop
    v.synchronize()
    prof = v.profile()
    v.profile_enable(False)

    # ---- What the library's DEFAULT (rgc_set_knn_reuse: seeds + neighbour lists) gives on this sequence -- extra keys, each timed exactly
    # like `value`: W warm-up steps and the K timed steps on two contexts from the same start, median of three passes.  `value` above keeps
    # nothing from step to step.  (a) the synthetic sequence as it is: a world-frame map that never changes; (b) seeds only; (c) one
    # coordinate of one point moved by an ulp before every frame: the library finds the map changed, searches everything (seeded) and
    # rebuilds its lists; (d) a keyframe every third frame: 1 % of the map's rows overwritten with points of that sweep in the world frame
    # (an insert + an evict, RGC_odometer.cpp:1236-1247), the two frames in between unchanged.  (c) and (d) are compared, bit for bit,
    # with the same edited sequence under RGC_REUSE_NONE.
    n_map = tgt.shape[0]
    map_host = np.zeros((n_map, 4), np.float32)
    map_host[:, :3] = maps[0]
    n_frames_all = K + W + 1
    one_np = torch.zeros((n_frames_all, 4), dtype=torch.float32).pin_memory().numpy()
    zz = np.float32(maps[0][7, 2])
    for i in range(n_frames_all):
        zz = np.nextafter(zz, np.float32(1e9))
        one_np[i, :3] = maps[0][7]
        one_np[i, 2] = zz
    kf_n = max(1, n_map // 100)
    n_slots = max(1, n_map // kf_n)
    n_kf = (n_frames_all + 2) // 3
    kf_np = torch.zeros((n_kf, kf_n, 4), dtype=torch.float32).pin_memory().numpy()
    kf_short = []
    map_lo, map_hi = maps[0].min(axis=0) + np.float32(0.5), maps[0].max(axis=0) - np.float32(0.5)
    alt = synth.make_map(world, None, seed=seed + 77)   # the same surfaces sampled again
    # (the blocks nearest to the vehicle first: the slabs the scans actually fall into, so that the edits reach the poses)
    cen = map_host[:n_slots * kf_n, :3].reshape(n_slots, kf_n, 3).mean(axis=1)
    slot_order = np.argsort(np.linalg.norm(cen - np.asarray(poses[0], np.float64)[:3, 3].astype(np.float32), axis=1))
    for kk in range(n_kf):
        i = min(3 * kk, len(scans) - 1)
        P = np.asarray(poses[i + 1], np.float64)
        # a keyframe RE-OBSERVES a region: the block of map rows it overwrites -- the map's rows are in leaf order, a block of them is a slab of the
        # world -- gets NEW samples of the same slab at the same density: the corresponding rows of an independent sampling of the same surfaces
        # (other jitter, other noise; the same leaf order).  What was tried first, and why not (EXPERIMENTS.md, round 6): a raw sweep (hundreds
        # of points per cell next to the sensor), a leaf-filtered sweep (isolated far returns: thousands of deferred queries), a sweep's points
        # over a slab (a hole in the ground), new samples near the vehicle against rows evicted all over a row-shuffled map (density drift, and
        # a shuffled map costs the counting sort its coherence) -- each changes what a frame costs by more than the turnover this key is about.
        slot = int(slot_order[kk % n_slots]) * kf_n
        a_lo = min(int(slot * (len(alt) / float(n_map))), max(0, len(alt) - kf_n))
        wpts = alt[a_lo:a_lo + kf_n]
        # (returns beyond the map's own bounding box are left out: rgc_set_target_reframed derives the re-framed map's box from the buffer's,
        # measured once per buffer -- "fixed between calls", rgc_hip.h; a rolling map that GROWS is the resident map's business, rgc_map_*)
        wpts = wpts[np.all((wpts > map_lo) & (wpts < map_hi), axis=1)]
        kf_np[kk, :wpts.shape[0], :3] = wpts
        kf_short.append(int(wpts.shape[0]))   # (a short keyframe: the rest of its block keeps the map's own rows, filled in below)
    def edit_one(i, w):
        w.upload_async(seq.d_map + 7 * 16, one_np[i:i + 1])
    for kk, got in enumerate(kf_short):   # (rows a short keyframe leaves alone keep the map's own points)
        if got < kf_n:
            slot = int(slot_order[kk % n_slots]) * kf_n
            kf_np[kk, got:, :] = map_host[slot + got:slot + kf_n]
    def edit_kf(i, w):
        if i % 3 == 0:
            w.upload_async(seq.d_map + int(slot_order[(i // 3) % n_slots]) * kf_n * 16, kf_np[i // 3])
    def timed_like_value(edit=None, overlap=True, reps=3):
        per, first, same = [], None, True
        sq = seq
        for _ in range(reps):
            if edit is not None:
                v.upload(seq.d_map, map_host)   # (synchronises) every pass starts from the map as generated
            Tw_s, g_s = Tw_init, I4
            if W > 0:
                m, wd, _ = sq.run(0, W, Tw_init, I4, overlap, edit_map=edit)
                Tw_s, g_s = wd[-1], m[-1]
            pv.synchronize()
            tr = time.perf_counter()
            m, _, _ = sq.run(W, K, Tw_s, g_s, overlap, edit_map=edit)
            pv.synchronize()
            per.append(time.perf_counter() - tr)
            if first is None:
                first = m
            else:
                same = same and all(np.array_equal(a_, b_) for a_, b_ in zip(first, m))
        return float(np.median(per)), first, same
    def rate(el):
        return {"scans_per_s": round(K / el, 3), "ms_per_step": round(1e3 * el / K, 4)}
    reuse = {}
    el_none_one, m_none_one, _ = timed_like_value(edit_one)
    el_none_kf, m_none_kf, _ = timed_like_value(edit_kf)
    v.upload(seq.d_map, map_host)
    for w in pv.v:
        w.setNeighbourReuse(REUSE_SEEDS)
    el, m_, sm = timed_like_value()
    reuse["seeds_only_unchanged_map"] = dict(rate(el), same_poses_as_value=bool(sm and all(np.array_equal(a_, b_) for a_, b_ in zip(motions, m_))))
    for w in pv.v:
        w.setNeighbourReuse(REUSE_LISTS)
    el, m_, sm = timed_like_value()
    el1, m1_, sm1 = timed_like_value(overlap=False)
    reuse["unchanged_map"] = dict(rate(el), one_frame_at_a_time=rate(el1),
                                  same_poses_as_value=bool(sm and sm1 and all(np.array_equal(a_, b_) for a_, b_ in zip(motions, m_))
                                                           and all(np.array_equal(a_, b_) for a_, b_ in zip(motions, m1_))),
                                  queries_searched_per_launch=int(pv.v[(K - 1) % 2].stats()["searched_target"]))
    el, m_, sm = timed_like_value(edit_one)
    reuse["one_point_edited_every_frame"] = dict(rate(el), with_nothing_kept=rate(el_none_one),
                                                 same_poses_as_with_nothing_kept=bool(sm and all(np.array_equal(a_, b_) for a_, b_ in zip(m_none_one, m_))))
    el, m_, sm = timed_like_value(edit_kf)
    reuse["keyframe_every_3rd_frame"] = dict(rate(el), with_nothing_kept=rate(el_none_kf), points_replaced_per_keyframe=int(kf_n),
                                             same_poses_as_with_nothing_kept=bool(sm and all(np.array_equal(a_, b_) for a_, b_ in zip(m_none_kf, m_))),
                                             poses_differ_from_the_unedited_sequence=bool(any(not np.array_equal(a_, b_) for a_, b_ in zip(motions, m_))))
    v.upload(seq.d_map, map_host)
    # the map's launch alone under the default: unchanged map (lists), and after a write to the buffer (everything searched, seeded, lists rebuilt)
    v.profile_enable(True)
    v.profile_select([DOMINANT])
    seq.frame_target(v, Tw_start)
    seq.frame_target(v, Tw_start)
    v.synchronize()
    v.profile_reset()
    for j in range(5):
        seq.frame_target(v, worlds[j % len(worlds)])
        v.synchronize()
    dom_lists = v.profile()[DOMINANT]
    v.profile_reset()
    for j in range(5):
        v.upload(seq.d_map + 7 * 16, one_np[j:j + 1])
        seq.frame_target(v, worlds[j % len(worlds)])
        v.synchronize()
    dom_rebuild = v.profile()[DOMINANT]
    v.profile_enable(False)
    v.upload(seq.d_map, map_host)
    reuse["map_knn_launch_alone_ms"] = {"unchanged_map_lists": round(dom_lists["total_ms"] / max(dom_lists["launches"], 1), 4),
                                        "after_a_write_seeded_search_and_lists_rebuilt": round(dom_rebuild["total_ms"] / max(dom_rebuild["launches"], 1), 4)}
    reuse["what"] = ("rgc_set_knn_reuse(RGC_REUSE_LISTS), the library's default, instead of `value`'s RGC_REUSE_NONE; every entry W warm-up + K timed steps on two "
                     "contexts, median of 3 passes.  unchanged_map: this synthetic sequence as it is (the world-frame map handed over bit for bit every frame -- "
                     "a caller that has dropped the reference's per-frame body-frame leaf filter of the sub-map, RGC_odometer.cpp:985-991); "
                     "one_point_edited_every_frame: one coordinate moved by an ulp before every frame (all-or-nothing invalidation: everything searched, seeded, "
                     "lists rebuilt); keyframe_every_3rd_frame: every third frame 1 % of the map's points (a block of rows = a slab of the world) is overwritten with NEW samples "
                     "of the same slab at the same density -- a keyframe that re-observes a region: an insert and an evict (RGC_odometer.cpp:1236-1247) at stationary statistics.  with_nothing_kept: the same edited sequence under RGC_REUSE_NONE (the edits' uploads included)")
    for w in pv.v:
        w.setNeighbourReuse(REUSE_NONE)

    checksum, rank_checksums = pose_checksums(np, worlds, world_size, dist)   # (after every timed region)
    if rank != 0:
        if world_size > 1:
            dist.destroy_process_group()
        return

    pf = np.asarray(per_frame, dtype=np.float64)
    mean_outer, mean_lin, mean_err, mean_corr, n_vox, t_cells, s_cells, def_src, def_tgt = pf.mean(axis=0)
    scans_per_s = K * world_size / elapsed
    B = algorithmic_bytes(args.n_source, args.n_target, n_vox, mean_corr, mean_lin, mean_err)

    # dominant kernel: checked against the all-stages pass (largest summed HIP-event time), measured over the timed region
    name = max(prof.items(), key=lambda kv: kv[1]["total_ms"])[0]
    if name != DOMINANT:
        log(f"warning: the breakdown pass names {name} as dominant, the timed region bracketed {DOMINANT}")
    name, d = DOMINANT, prof_dom
    per_unit = 36.0  # 12 B read + 24 B written per point of the kNN / covariance stage
    avg_ms = d["total_ms"] / max(d["launches"], 1)
    units = d["points"] / max(d["launches"], 1)
    achieved = per_unit * units / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
    pmc, pmc_src = profile_json(PMC_FILE)  # rocprofv3 --pmc passes of this kernel (scripts/pmc_kernel.sh), if committed
    traffic = pmc.get("hbm_bytes_per_launch") if pmc else None
    # The same kernel against the roof that binds it -- VALU instruction issue.  Peaks are MEASURED (scripts/ubench/valu_issue.hip,
    # profiles/r02_valu_issue.jsonl, 8 waves per SIMD, every CU): add / sub / mul / fma / and / or / mov issue at ~1060 G
    # wave-instructions/s chip-wide (the 2-cycles-per-wave64 figure of the guide, 1229 G/s at 2.4 GHz, less the clock held under
    # load); min / max / med3 / compare / select / shifts / three-operand integer ops and ALL fp64 at ~595 G/s -- half rate.  The
    # peak a kernel can reach is the one of ITS mix: full- and half-rate instructions counted in the kernel's ISA, weighted by the
    # blocks' execution (scripts/isa_mix.py -> profiles/*_isa_mix.json); time per instruction adds, so the peaks combine harmonically.
    issue = None
    if pmc and avg_ms > 0 and pmc.get("valu_wave_instructions_per_query"):
        per_q = float(pmc["valu_wave_instructions_per_query"])
        ach = per_q * units / (avg_ms * 1e-3) / 1e9
        issue = {"bound": "valu_issue", "kernel": name, "achieved": round(ach, 1), "unit": "G wave-instr/s", "valu_wave_instructions_per_query": per_q,
                 "peak_full_rate_measured": 1060.0, "peak_half_rate_measured": 595.0, "peak_2cyc_at_2.4GHz": 1228.8}
        issue["valu_per_query_source"] = pmc_src
        mix, mix_src = profile_json(MIX_FILE)
        if pmc.get("launch") != "full_search":  # (the counters must be those of the launch `value` runs)
            mix = None
            issue["what"] = "the committed counters are not those of the full search: no mix-weighted peak"
        if mix and mix.get("half_rate_fraction") is not None:
            issue["half_rate_fraction_source"] = mix_src
            h = float(mix["half_rate_fraction"])
            peak = 1.0 / (h / 595.0 + (1.0 - h) / 1060.0)
            issue.update({"half_rate_fraction": round(h, 4), "peak_mix_weighted": round(peak, 1), "frac_of_mix_weighted_peak": round(ach / peak, 4),
                          "frac_of_mix_weighted_peak_launch_alone": None})
    roofline = {"bound": "hbm", "kernel": name, "achieved": round(achieved, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 6), "traffic": traffic, "traffic_source": pmc_src,
                "avg_launch_ms": round(avg_ms, 4), "algorithmic_bytes_per_launch": per_unit * units}
    # the whole frame's MEASURED HBM bytes (every kernel of a dependent frame, FETCH_SIZE x 2 + WRITE_SIZE) against the algorithmic B
    ft, ft_src = profile_json(FRAME_TRAFFIC_FILE)
    frame_traffic = None
    if ft and ft.get("bytes_per_frame_measured"):
        frame_traffic = {"bytes_per_frame_measured": int(ft["bytes_per_frame_measured"]), "algorithmic_bytes_per_scan": round(B),
                         "measured_over_algorithmic": round(float(ft["bytes_per_frame_measured"]) / B, 3), "source": ft_src,
                         "largest": [{k: r[k] for k in ("kernel", "MB_per_frame")} for r in ft.get("per_kernel", [])[:5]]}
    alone_ms = dom_alone["total_ms"] / max(dom_alone["launches"], 1)
    if alone_ms > 0:  # the timed region runs the launch beside the next scan's kernels; alone it is shorter
        roofline["launch_alone_ms"] = round(alone_ms, 4)
        roofline["frac_launch_alone"] = round(per_unit * units / (alone_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 6)
        roofline["queries_searched_per_launch"] = searched_alone
        roofline["what"] = ("the map's bulk exact 20-NN + covariance launch, every one of its queries searched in full (rgc_set_knn_reuse(RGC_REUSE_NONE): "
                            "the launch of a map the library has not seen, k_knn_sp<20, true, true, false>) -- the longest kernel of the timed frame "
                            "(roofline_by_kernel); achieved = 36 B x points / the launch's own start-to-stop time (hipExtLaunchKernelGGL events on its "
                            "stream) averaged over the timed region; launch_alone_ms from a pass with nothing else on the GPU; traffic = measured HBM "
                            "bytes of this launch (rocprofv3 --pmc FETCH_SIZE x 2 + WRITE_SIZE, separate passes, traffic_source).  The launches of the "
                            "library's default mode are under reuse_of_an_unchanged_map")
        if issue and issue.get("peak_mix_weighted"):
            issue["frac_of_mix_weighted_peak_launch_alone"] = round(issue["valu_wave_instructions_per_query"] * units / (alone_ms * 1e-3) / 1e9
                                                                    / issue["peak_mix_weighted"], 4)
    # the five kernels with the most GPU time in a frame of the timed workload, each against ITS algorithmic bytes (SURVEY 8d's
    # terms where 8d has one, the kernel's own minimum where it has none -- the grid build), with the measured traffic beside it.  GPU time and
    # traffic per frame come from committed rocprofv3 passes over the same workload (stamped); the live per-stage HIP-event times of THIS run
    # are in kernel_ms_per_step.
    by_kernel = roofline_by_kernel(args.n_source, args.n_target, n_vox, mean_corr, t_cells, s_cells, def_src, ft)

    out = headline(args, K, W, world_size, elapsed, step_stamps, PREWARM, searched_alone, host_loop, checksum, rank_checksums, np)
    out.update({
        "algorithmic_bytes_per_scan": round(B), "hbm_gbps_algorithmic": round(B * scans_per_s / world_size / 1e9, 3),
        "hbm_frac_whole_frame": round(B * scans_per_s / world_size / 1e9 / HBM_PEAK_GBS, 6),
        "mean_outer_iterations": round(mean_outer, 2), "mean_linearize": round(mean_lin, 2), "mean_compute_error": round(mean_err, 2),
        "mean_correspondences": round(mean_corr, 1), "n_voxels": int(n_vox),
        "kernel_ms_per_step": {k: round(x["total_ms"] / KB, 4) for k, x in prof.items()},
        "roofline": roofline, "roofline_by_kernel": by_kernel, "issue_roofline": issue, "frame_traffic": frame_traffic,
        "one_frame_at_a_time": {"scans_per_s": round(K / elapsed_seq, 3), "ms_per_step": round(1e3 * elapsed_seq / K, 3), "same_poses": seq_same,
                                "what": "the same K dependent steps on one context through the blocking calls: a frame's latency"},
        "replay_of_preframed_maps": {"scans_per_s": round(K / elapsed_replay, 3), "ms_per_step": round(1e3 * elapsed_replay / K, 3),
                                     "max_abs_pose_difference_to_the_dependent_run": replay_err,
                                     "what": "targets that do NOT depend on the previous pose (three translated copies of the map in turn): a whole frame's "
                                             "preparation overlaps the previous solve -- round 2's `value`; a replay of pre-framed sub-maps, not a live sequence"},
        "scan_h2d_and_output": {"scans_per_s": round(K / elapsed_h2d, 3), "ms_per_step": round(1e3 * elapsed_h2d / K, 3), "same_final_pose": h2d_same,
                                "what": "the dependent steps; each scan uploaded from pinned host memory inside the step, align()'s output cloud written to a device buffer"},
        "steady_state": steady, "lazy_target": lazy, "reuse_of_an_unchanged_map": reuse,
    })

    oracle = None
    if world_size == 1 and not args.no_cpu_baseline:
        # CPU baseline: the oracle (a port; the reference itself cannot be built here) on this box's host cores, on a bounded sample of
        # the same workload -- re-framing of the map (B9), target and source preparation, solve, fitness -- and the parity check of those
        # frames: each from the GPU path's own previous pose and guess, registered to the SAME target cloud (the re-framed map is
        # downloaded, so the two paths see identical inputs; the oracle's own B9 is timed, its output agrees to 4e-6, tests/test_gpu_pre.py).
        from oracle import oracle
        cores = os.cpu_count() or 1
        # at the reference's own thread count (setNumThreads(14), RGC_odometer.cpp:1006): on a many-core host more OpenMP threads make
        # this path SLOWER (its parallel loops are short), so this is also the faster setting; one frame on all cores is timed beside it
        nthr = min(14, cores)
        o = oracle.Registration(num_threads=nthr)
        n_done, t_cpu, dts, dths = 0, 0.0, [], []
        map_xyzi = np.zeros((tgt.shape[0], 4), np.float32)
        map_xyzi[:, :3] = tgt
        for j in range(K):
            Tw_prev = Tw_start if j == 0 else worlds[j - 1]
            q, t = world_to_body(Tw_prev)
            v.transformCloudDevice(d_maps[0], tgt.shape[0], 16, q, t, seq.d_body[id(v)])
            tgt_j = v.download(seq.d_body[id(v)], (tgt.shape[0], 4))[:, :3].copy()
            c0 = time.perf_counter()
            _ = oracle.transform_cloud(map_xyzi, q, t)   # the oracle's own B9: timed
            o.set_target(tgt_j)
            o.set_source(scans[W + j])
            To = o.align(guesses[j])
            _ = o.fitness()
            t_cpu += time.perf_counter() - c0
            Tg = motions[j]
            dts.append(float(np.abs(Tg[:3, 3] - To[:3, 3]).max()))
            dths.append(rot_angle(Tg[:3, :3], To[:3, :3]))
            n_done += 1
            if t_cpu > 20.0:  # bounded: all timed frames (~0.25 s each) or 20 s of CPU work
                break
        out["cpu_baseline"] = {"value": round(n_done / t_cpu, 4), "unit": "scans/s", "cores": nthr, "kind": "port",
                               "sample": f"{n_done} frame(s) of the same workload (first timed frames, each from the GPU path's own previous pose and guess), "
                                         f"OpenMP x{nthr} (the reference's setNumThreads), {t_cpu:.1f} s of CPU work"}
        if cores > nthr:
            oa = oracle.Registration(num_threads=cores)
            c0 = time.perf_counter()
            oa.set_target(tgt_j)
            oa.set_source(scans[W + n_done - 1])
            oa.align(guesses[n_done - 1])
            _ = oa.fitness()
            ta = time.perf_counter() - c0
            out["cpu_baseline"]["value_all_cores"] = round(1.0 / ta, 4)
            out["cpu_baseline"]["sample"] += f"; 1 frame at {cores} threads, {ta:.1f} s"
        out["pose_parity_vs_cpu"] = {"frames": n_done, "max_dt_m": max(dts), "max_dtheta_rad": max(dths),
                                     "rmse_dt_m": float(np.sqrt(np.mean(np.square(dts)))),
                                     "rmse_dtheta_rad": float(np.sqrt(np.mean(np.square(dths))))}
    if world_size == 1 and not args.no_two_sequences:
        K2 = min(K, 20)
        world_b, tgt_b = synth.make_world_and_map(args.n_target, seed=seed + 1)
        poses_b, scans_b = make_sequence(synth, world_b, K2 + W, args.n_source, seed + 1)
        out["two_sequences_per_gpu"] = two_sequences_per_gpu(registration, synth, np, device_index, seq, pv, tgt.shape[0], args.n_source, seed, W,
                                                             K2, Tw_init, I4, second=(tgt_b, poses_b, scans_b))
        try:
            out["sequences_per_gpu"] = sequences_per_gpu(np, device_index, [(tgt, poses[0], scans), (tgt_b, poses_b[0], scans_b)], min(K2 + W, len(scans_b)))
            B1 = out["algorithmic_bytes_per_scan"]
            for x in out["sequences_per_gpu"].get("runs", []):
                x["hbm_gbps_algorithmic"] = round(B1 * x["aggregate_scans_per_s"] / 1e9, 1)
                x["hbm_frac_algorithmic"] = round(B1 * x["aggregate_scans_per_s"] / 1e9 / HBM_PEAK_GBS, 5)
        except Exception as e:   # the metric line must not be lost to a side measurement
            out["sequences_per_gpu"] = {"error": str(e)[:300]}
    seq.close()
    pv.close()

    if world_size == 1 and args.configs != "none":
        out["configs"] = run_extra_configs(registration, synth, oracle, [c.strip() for c in args.configs.split(",") if c.strip()])

    print(json.dumps(out), flush=True)
    if world_size > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
