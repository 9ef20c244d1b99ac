"""4-DoF pose-graph optimisation over a keyframe store's key poses -- host-side mirror of the rgc_pgo_* entry points of include/rgc_hip.h:
the mapping node's PoseGraphOptimize4DoF (src/RGC_mapping.cpp:2303-2466), the link between a loop-closure ICP's drift matrix and the
store's poses.

    graph = PoseGraph4DoF(store)
    graph.loop_from_icp(key_curr, pose_curr, key_loop, pose_loop, T_drift)   # rgc_icp_align's final_T -> a loop edge (:2086-2107)
    report, poses = graph.optimize(ids)                       # the store's poses are corrected (apply=True)
    global_map = store.assemble(ids, (KF_CORNER, KF_SURF), leaf=0.4)

The system is linearised and solved on the device; nothing is computed on the CPU but the LM decisions.  Without librgc_hip.so / an
MI355X this raises."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import PGO_OPTIMIZED, PGO_NO_LOOP, RgcError  # noqa: F401  (re-exported)

_ip = C.POINTER(C.c_int)
_dp = C.POINTER(C.c_double)
STOP_NAMES = ("cap", "gradient", "function", "parameter", "radius")


def make_loop(latest_pose, loop_pose, T_drift, key_curr, key_loop) -> _lib.PgoLoop:
    """rgc_pgo_make_loop (host only): poses (x, y, z, roll, pitch, yaw) float32, T_drift 4x4"""
    a = np.ascontiguousarray(latest_pose, np.float32).reshape(6)
    b = np.ascontiguousarray(loop_pose, np.float32).reshape(6)
    T = np.ascontiguousarray(T_drift, np.float32).reshape(16)
    out = _lib.PgoLoop()
    rc = _lib.load().rgc_pgo_make_loop(a.ctypes.data_as(C.POINTER(_lib.KfPose)), b.ctypes.data_as(C.POINTER(_lib.KfPose)),
                                       T.ctypes.data_as(C.POINTER(C.c_float)), int(key_curr), int(key_loop), C.byref(out))
    if rc:
        raise RgcError(rc, "rgc_pgo_make_loop: a pose or the drift is not finite")
    return out


def _report(r: _lib.PgoReport) -> dict:
    return dict(status=r.status, n_nodes=r.n_nodes, n_odom=r.n_odom, n_loops_used=r.n_loops_used, n_loops_ignored=r.n_loops_ignored,
                fixed_id=r.fixed_id, iterations=r.iterations, successful=r.successful, stop=STOP_NAMES[r.stop],
                accepted=[bool((r.accepted_mask >> k) & 1) for k in range(r.iterations)], initial_cost=r.initial_cost, final_cost=r.final_cost)


class PoseGraph4DoF:
    """The loops of a pose graph over ``store`` (a ``keyframes.KeyframeStore``); the nodes and the odometry edges are the store's poses."""

    def __init__(self, store):
        self._store = store
        self._L = store._L
        self.loops: list[_lib.PgoLoop] = []

    def add_loop(self, key_curr, key_loop, t_loop_curr, yaw_loop_curr_deg, pitch_loop_deg, roll_loop_deg):
        l = _lib.PgoLoop(int(key_curr), int(key_loop), (C.c_double * 3)(*[float(v) for v in t_loop_curr]), float(yaw_loop_curr_deg),
                         float(pitch_loop_deg), float(roll_loop_deg))
        self.loops.append(l)
        return l

    def loop_from_icp(self, key_curr, latest_pose, key_loop, loop_pose, T_drift):
        """the edge of a closed loop: the two key poses as they were when the ICP ran, and its final transformation"""
        l = make_loop(latest_pose, loop_pose, T_drift, key_curr, key_loop)
        self.loops.append(l)
        return l

    def _args(self, ids):
        i = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        n = len(self.loops)
        arr = (_lib.PgoLoop * max(n, 1))(*self.loops)
        return i, i.ctypes.data_as(_ip) if i.shape[0] else None, arr if n else None, n

    def optimize(self, ids, apply=True, max_iterations=None, initial_radius=None):
        """rgc_pgo_optimize over the keyframes ``ids`` in that order: (report dict, corrected poses (n, 6) float32)"""
        i, ipp, arr, n = self._args(ids)
        prm = _lib.PgoParams()
        self._L.rgc_default_pgo_params(C.byref(prm))
        if max_iterations is not None:
            prm.max_iterations = int(max_iterations)
        if initial_radius is not None:
            prm.initial_radius = float(initial_radius)
        out = np.zeros((i.shape[0], 6), np.float32)
        rep = _lib.PgoReport()
        self._store._chk(self._L.rgc_pgo_optimize(self._store._h, ipp, i.shape[0], arr, n, C.byref(prm), 1 if apply else 0,
                                                  out.ctypes.data_as(C.POINTER(_lib.KfPose)), C.byref(rep)))
        return _report(rep), out

    def linearize(self, ids, x_eval=None, radius=0.0):
        """rgc_pgo_linearize: dict(edge_ij (E, 2), edge_meas (E, 6), residuals (E, 4), g (N, 4), cost, H_diag (N, 4, 4), H_chain (N - 1, 4, 4),
        H_loop (L, 4, 4), d (N, 4) or None, report)"""
        i, ipp, arr, n = self._args(ids)
        N = i.shape[0]
        rep = _lib.PgoReport()
        x = None if x_eval is None else np.ascontiguousarray(x_eval, np.float64).reshape(N, 4)
        xp = None if x is None else x.ctypes.data_as(_dp)
        E = N - 1 + n                       # room for every loop; the report says how many were used
        ij = np.zeros((max(E, 1), 2), np.int32)
        meas, res = np.zeros((max(E, 1), 6)), np.zeros((max(E, 1), 4))
        g, Hd, Hc, Hl, d = np.zeros((N, 4)), np.zeros((N, 4, 4)), np.zeros((max(N - 1, 1), 4, 4)), np.zeros((max(n, 1), 4, 4)), np.zeros((N, 4))
        cost = C.c_double(0.0)
        p = lambda a: a.ctypes.data_as(_dp)   # noqa: E731
        self._store._chk(self._L.rgc_pgo_linearize(self._store._h, ipp, N, arr, n, xp, float(radius), ij.ctypes.data_as(_ip), p(meas), p(res), p(g), C.byref(cost),
                                                   p(Hd), p(Hc), p(Hl), p(d), C.byref(rep)))
        Lu = rep.n_loops_used
        E = N - 1 + Lu
        return dict(edge_ij=ij[:E], edge_meas=meas[:E], residuals=res[:E], g=g, cost=cost.value, H_diag=Hd, H_chain=Hc[:N - 1], H_loop=Hl[:Lu],
                    d=d if radius > 0 and Lu > 0 else None, report=_report(rep))
