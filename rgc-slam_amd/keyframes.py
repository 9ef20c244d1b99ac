"""f5: the mapping node's keyframe store kept resident on the device -- host-side mirror of the rgc_kf_* entry points of include/rgc_hip.h.
Replaces the three places where the mapping node assembles a cloud from its keyframes with transformPointCloud per keyframe, `+=` and a
pcl::VoxelGrid (src/RGC_mapping.cpp:1503-1616 the surrounding maps of f1, :2180-2216 source and target of f4, :2508-2537 the global map):

    store = KeyframeStore(icp)                               # lives in the context of the object that consumes its clouds (or its own)
    store.push(key_id, pose, corner, surf, scan)             # body-frame clouds (n, >=4) float32; pose = (x, y, z, roll, pitch, yaw), radians
    store.set_poses(ids, poses)                              # correctKeyFramePoseGraph (:1618-1686)
    target = store.assemble(history_ids, (KF_CORNER, KF_SURF), leaf=0.4, device=True)
    icp.setInputTarget(target)                               # rgc_icp_align_device: no download, no upload

and with the three places where it finds WHICH keyframes to assemble with a kd-tree over the key poses and a pcl::UniformSampling
(:1525-1548, 2141-2225, 2493-2505):

    near = store.select_surrounding(position, 15.0, 0.3)     # ids: key poses within 15 m, thinned at 0.3 m
    loop = store.detect_loop()                               # found, latest_id, closest_id, the poses, history_ids (the ICP target's keyframes)
    everything = store.select_global(0.5)                    # ids of the global map's keyframes
    distance, angle = store.travel(ids)                      # travelled distance / angle per keyframe, fixed at its push (:1887-1908)

Nothing is computed on the CPU; without librgc_hip.so / an MI355X this raises."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import KF_CORNER, KF_SURF, KF_SCAN, RgcError  # noqa: F401  (re-exported)

_ip = C.POINTER(C.c_int)


def _poses(poses):
    p = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 6)
    return p, p.ctypes.data_as(C.POINTER(_lib.KfPose))


class DeviceCloud:
    """(n, 4) float32 points {x, y, z, c} in device memory of the context that assembled them; what ``assemble(device=True)`` returns and
    ``IterativeClosestPoint.setInputSource / setInputTarget`` and ``MapFeatureRegistration.setInputMaps`` accept.  Frees its buffer with
    ``close()`` (or when collected); the context must still be alive then."""

    def __init__(self, L, h, ptr, n, n_raw, cap):
        self._L, self._h, self.ptr, self.n, self.n_raw, self.cap = L, h, ptr, int(n), int(n_raw), int(cap)

    def __len__(self):
        return self.n

    @property
    def stride_bytes(self):
        return 16

    def synchronize(self):
        """wait for the assembly (a consumer on ANOTHER context of the same device calls this; on the same context stream order does)"""
        rc = self._L.rgc_synchronize(self._h)
        if rc:
            raise RgcError(rc, self._L.rgc_last_error(self._h).decode())

    def numpy(self):
        out = np.empty((self.n, 4), np.float32)
        if self.n:
            rc = self._L.rgc_download(self._h, out.ctypes.data, self.ptr, out.nbytes)
            if rc:
                raise RgcError(rc, self._L.rgc_last_error(self._h).decode())
        return out

    def close(self):
        if self.ptr:
            self._L.rgc_device_free(self._h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KeyframeStore:
    """``owner``: an object with a context (``FastVGICP``, ``IterativeClosestPoint``, ``MapFeatureRegistration``) whose stream the store's
    work is ordered on, or None for a context of the store's own on ``device``."""

    def __init__(self, owner=None, device: int = 0):
        self._L = _lib.load()
        self._own = owner is None
        if owner is None:
            h = C.c_void_p()
            rc = self._L.rgc_create(device, None, C.byref(h))
            if rc:
                raise RgcError(rc, self._L.rgc_status_string(rc).decode())
            self._h = h
        else:
            self._h = owner._h
            self._owner = owner   # keeps the context alive

    def close(self):
        if self._own and getattr(self, "_h", None):
            self._L.rgc_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise RgcError(rc, self._L.rgc_last_error(self._h).decode() or self._L.rgc_status_string(rc).decode())

    def reset(self):
        self._chk(self._L.rgc_kf_reset(self._h))

    def push(self, key_id, pose, corner=None, surf=None, scan=None):
        clouds, stride = [], None
        for a in (corner, surf, scan):
            if a is None or len(a) == 0:
                clouds.append((None, 0))
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] < 4:
                raise RgcError(_lib.ERR_INVALID, "a keyframe cloud is (n, >=4) float32: x, y, z, c")
            if stride not in (None, a.strides[0]):
                raise RgcError(_lib.ERR_INVALID, "the clouds of one keyframe must have the same point layout")
            stride = a.strides[0]
            clouds.append((a, a.shape[0]))
        p, pp = _poses(pose)
        (c, nc), (s, ns), (k, nk) = clouds
        self._chk(self._L.rgc_kf_push(self._h, int(key_id), pp, c.ctypes.data if nc else None, nc, s.ctypes.data if ns else None, ns,
                                      k.ctypes.data if nk else None, nk, stride or 16, 0))

    def set_poses(self, ids, poses):
        i = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        p, pp = _poses(poses)
        if p.shape[0] != i.shape[0]:
            raise RgcError(_lib.ERR_INVALID, "one pose per id")
        self._chk(self._L.rgc_kf_set_poses(self._h, i.ctypes.data_as(_ip), pp, i.shape[0]))

    def info(self) -> dict:
        i = _lib.KfInfo()
        self._chk(self._L.rgc_kf_get_info(self._h, C.byref(i)))
        return dict(n_keyframes=i.n_keyframes, n_points=list(i.n_points), revision=i.revision)

    def travel(self, ids):
        """(distance, angle) float32 arrays: the travelled distance and accumulated |yaw change| up to each keyframe, fixed at its push
        (src/RGC_mapping.cpp:1887-1908)"""
        i = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        d, a = np.zeros(i.shape[0], np.float32), np.zeros(i.shape[0], np.float32)
        fp = C.POINTER(C.c_float)
        self._chk(self._L.rgc_kf_get_travel(self._h, i.ctypes.data_as(_ip) if i.shape[0] else None, i.shape[0], d.ctypes.data_as(fp), a.ctypes.data_as(fp)))
        return d, a

    def _n(self):
        return self.info()["n_keyframes"]

    def select_surrounding(self, center, radius=15.0, density=0.3, return_count=False):
        """extractSurroundingKeyFramesAndMap's selection (:1525-1548): the ids of the key poses strictly within ``radius`` of ``center``, thinned by
        UniformSampling at leaf ``density``, in ascending leaf index; with ``return_count`` also the number of poses inside the radius"""
        q = np.ascontiguousarray(center, dtype=np.float32).ravel()
        if q.shape[0] != 3:
            raise RgcError(_lib.ERR_INVALID, "the centre is (x, y, z)")
        cap = self._n()
        out = np.empty(max(cap, 1), np.int32)
        nin, no = C.c_int(0), C.c_int(0)
        self._chk(self._L.rgc_kf_select_surrounding(self._h, q.ctypes.data_as(C.POINTER(C.c_float)), float(radius), float(density), out.ctypes.data_as(_ip), cap,
                                                    C.byref(nin), C.byref(no)))
        ids = out[:no.value].copy()
        return (ids, nin.value) if return_count else ids

    def select_global(self, pose_density=0.5):
        """publishGlobalMap's selection (:2493-2505): UniformSampling of every key position at leaf ``pose_density``; ids in ascending leaf index"""
        cap = self._n()
        out = np.empty(max(cap, 1), np.int32)
        no = C.c_int(0)
        self._chk(self._L.rgc_kf_select_global(self._h, float(pose_density), out.ctypes.data_as(_ip), cap, C.byref(no)))
        return out[:no.value].copy()

    def detect_loop(self, **params):
        """detectLoopClosure (:2141-2225) for the last keyframe pushed.  ``params`` override rgc_default_kf_loop_params (history_search_radius,
        drift_factor, distance_by_loop, loop_keyframe_dis_diff, history_search_num, min_key_id).  Returns a dict: found, latest_id, closest_id,
        latest_pose, closest_pose (6 floats each), search_radius, n_in_radius, history_ids (int32 array, the target's keyframes in order)."""
        prm = _lib.KfLoopParams()
        self._L.rgc_default_kf_loop_params(C.byref(prm))
        for k, v in params.items():
            if k not in dict(_lib.KfLoopParams._fields_):
                raise RgcError(_lib.ERR_INVALID, f"no loop parameter {k}")
            setattr(prm, k, v)
        cap = min(self._n(), 2 * max(int(prm.history_search_num), 0) + 1)
        hist = np.empty(max(cap, 1), np.int32)
        cand, nh = _lib.KfLoopCandidate(), C.c_int(0)
        self._chk(self._L.rgc_kf_detect_loop(self._h, C.byref(prm), C.byref(cand), hist.ctypes.data_as(_ip), cap, C.byref(nh)))
        def pose(p):
            return np.array([p.x, p.y, p.z, p.roll, p.pitch, p.yaw], np.float32)

        return dict(found=bool(cand.found), latest_id=cand.latest_id, closest_id=cand.closest_id, latest_pose=pose(cand.latest_pose),
                    closest_pose=pose(cand.closest_pose), search_radius=float(cand.search_radius), n_in_radius=cand.n_in_radius,
                    history_ids=hist[:nh.value].copy())

    def optimize_pose_graph(self, ids, loops, apply=True, max_iterations=None, initial_radius=None):
        """PoseGraphOptimize4DoF (src/RGC_mapping.cpp:2303-2466) over the keyframes ``ids`` in one call: ``loops`` are ``_lib.PgoLoop`` records
        (``pose_graph.make_loop`` turns a loop-closure ICP's drift into one).  Returns (report dict, corrected poses (n, 6) float32); with
        ``apply`` the store's poses are corrected."""
        from .pose_graph import PoseGraph4DoF
        graph = PoseGraph4DoF(self)
        graph.loops = list(loops)
        return graph.optimize(ids, apply=apply, max_iterations=max_iterations, initial_radius=initial_radius)

    @staticmethod
    def kind_mask(kinds) -> int:
        if isinstance(kinds, (int, np.integer)):
            kinds = (int(kinds),)
        m = 0
        for k in kinds:
            if not 0 <= int(k) < _lib.KF_KINDS:
                raise RgcError(_lib.ERR_INVALID, f"no keyframe cloud kind {k}")
            m |= 1 << int(k)
        return m

    def assemble(self, ids, kinds, leaf=0.0, device=False):
        """The clouds of ``kinds`` of the keyframes ``ids``, in that order (kinds ascending inside a keyframe), under the current poses,
        through the leaf filter when ``leaf`` > 0: an (n, 4) float32 array, or a ``DeviceCloud`` when ``device``."""
        i = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        ipp = i.ctypes.data_as(_ip) if i.shape[0] else None
        mask = self.kind_mask(kinds)
        n_raw, n_out = C.c_int(0), C.c_int(0)
        # the counts first (no filter, no room: nothing runs on the device), then a buffer the unfiltered selection fits into
        rc = self._L.rgc_kf_assemble(self._h, ipp, i.shape[0], mask, 0.0, None, 0, 0, C.byref(n_raw), C.byref(n_out))
        if rc and n_raw.value == 0:
            self._chk(rc)
        cap = n_raw.value
        if device:
            d = C.c_void_p()
            self._chk(self._L.rgc_device_alloc(self._h, max(cap, 1) * 16, C.byref(d)))
            rc = self._L.rgc_kf_assemble(self._h, ipp, i.shape[0], mask, float(leaf), d, cap, 1, C.byref(n_raw), C.byref(n_out))
            if rc:
                self._L.rgc_device_free(self._h, d)
                self._chk(rc)
            return DeviceCloud(self._L, self._h, d, n_out.value, n_raw.value, cap)
        out = np.empty((cap, 4), np.float32)
        self._chk(self._L.rgc_kf_assemble(self._h, ipp, i.shape[0], mask, float(leaf), out.ctypes.data if cap else None, cap, 0, C.byref(n_raw), C.byref(n_out)))
        return out[:n_out.value]


def pose_of(T):
    """(x, y, z, roll, pitch, yaw) float32 of a 4x4 sensor->world pose with R = Rz(yaw) Ry(pitch) Rx(roll) (Utility::R2ypr's convention)"""
    R = np.asarray(T, np.float64)
    yaw = np.arctan2(R[1, 0], R[0, 0])
    pitch = np.arctan2(-R[2, 0], np.hypot(R[0, 0], R[1, 0]))
    roll = np.arctan2(R[2, 1], R[2, 2])
    return np.array([R[0, 3], R[1, 3], R[2, 3], roll, pitch, yaw], np.float32)


def synthetic_keyframes(n_keyframes, seed=None, n_az=600, every=3, device=0, scan_stride=4):
    """Keyframes of a synthetic drive (synth.make_world / make_trajectory / make_scan), as the mapping node would store them: per keyframe the
    front-end's sharp and flat features {x, y, z, normal_x} and a thinned sweep {x, y, z, intensity}, all in the BODY frame, and the key pose.
    Data for tests and scripts/bench_keyframes.py; the features come from the library's own front-end (needs the GPU).
    Returns (ids, poses (n, 6) float32, clouds {id: [corner, surf, scan]})."""
    from . import synth
    from .frontend import ScanRegistration
    seed = synth.SEED if seed is None else seed
    world = synth.make_world(seed=seed)
    traj = synth.make_trajectory(n_keyframes * every, seed=seed)[::every]
    fe = ScanRegistration(device=device)
    ids, poses, clouds = [], [], {}
    try:
        for i, T in enumerate(traj):
            sc = synth.make_scan(world, T, n_az=n_az, seed=seed + 10 + i)
            xyzi = np.concatenate([sc["xyz"], sc["intensity"][:, None]], axis=1).astype(np.float32)
            f = fe.laserCloudHandler(xyzi, diagnostics=False)
            ids.append(i)
            poses.append(pose_of(T))
            clouds[i] = [np.ascontiguousarray(f["sharp"][:, [0, 1, 2, 4]], np.float32), np.ascontiguousarray(f["flat"][:, [0, 1, 2, 4]], np.float32),
                         np.ascontiguousarray(f["cloud"][::scan_stride], np.float32)]
    finally:
        fe.close()
    return ids, np.array(poses, np.float32), clouds
