"""An independent numpy reference of the keyframe store's sub-map assembly (rgc_kf_assemble): no line of it is shared with the library.

The pose chain as the mapping node's transformPointCloud(cloud, &pose6D) writes it (src/RGC_mapping.cpp:2575-2581):
    float32 x, y, z, roll, pitch, yaw  ->  Vector3d(yaw, pitch, roll) * rad2deg in fp64 (rad2deg = 180.0 / M_PI, :197)
    ->  Utility::ypr2R in DEGREES (include/rgc_slam/utility.h:123-147: y = ypr(0) / 180.0 * M_PI ..., Rz * Ry * Rx)  ->  R * p + t
with everything after the fp64 `* rad2deg` evaluated in np.longdouble (64-bit mantissa on x86), the constants 180.0 and M_PI being the
doubles the reference's text names.  The concatenation: for each id in the order given, for each selected kind in ascending kind order, the
keyframe's points in stored order.  The leaf filter: tests/pre_reference.py's voxelgrid (imported, not modified)."""
import math

import numpy as np

import pre_reference as pr

LD = np.longdouble
KINDS = 3   # corner, surf, scan


def pose_f32(pose):
    """(x, y, z, roll, pitch, yaw) as the float32 fields of PointXYZIRPYT"""
    return np.asarray(pose, np.float32).reshape(6)


def rotation(pose):
    """3x3 longdouble: ypr2R(Vector3d(yaw, pitch, roll) * rad2deg)"""
    p = pose_f32(pose)
    rad2deg = np.float64(180.0) / np.float64(math.pi)
    deg = np.array([p[5], p[4], p[3]], np.float64) * rad2deg          # fp64, as the reference's expression types make it
    assert deg.dtype == np.float64
    y, pt, r = (deg.astype(LD) / LD(180.0)) * LD(np.float64(math.pi))
    cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(pt), np.sin(pt), np.cos(r), np.sin(r)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]], LD)
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]], LD)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]], LD)
    return Rz @ Ry @ Rx


def translation(pose):
    return pose_f32(pose)[:3].astype(np.float64).astype(LD)


def transform_cloud(points, pose):
    """R p + t of the (n, >= 3) float32 points, (n, 3) longdouble"""
    p = np.asarray(points, np.float32)[:, :3].astype(LD)
    return p @ rotation(pose).T + translation(pose)[None, :]


def kinds_of(mask):
    return [k for k in range(KINDS) if (mask >> k) & 1]


class Assembly:
    """xyz: (N, 3) longdouble; c: (N,) float32 fourth floats; p_abs / t_abs: (N,) |p| and |t| of every point's segment (for pr.ulp_bound);
    segments: (id, kind, first, count) in output order"""

    def __init__(self, xyz, c, p_abs, t_abs, segments):
        self.xyz, self.c, self.p_abs, self.t_abs, self.segments = xyz, c, p_abs, t_abs, segments

    @property
    def n(self):
        return self.xyz.shape[0]


def assemble(clouds, poses, ids, mask):
    """clouds: {id: [corner, surf, scan]} of (n, 4) float32 body-frame arrays (an empty kind: shape (0, 4)); poses: {id: 6 floats}"""
    xyz, c, pa, ta, segs, at = [], [], [], [], [], 0
    for i in ids:
        for k in kinds_of(mask):
            a = np.asarray(clouds[i][k], np.float32).reshape(-1, 4)
            if not len(a):
                continue
            xyz.append(transform_cloud(a, poses[i]))
            c.append(a[:, 3].copy())
            pa.append(np.linalg.norm(a[:, :3].astype(np.float64), axis=1))
            ta.append(np.full(len(a), float(np.linalg.norm(translation(poses[i]).astype(np.float64)))))
            segs.append((i, k, at, len(a)))
            at += len(a)
    if not xyz:
        return Assembly(np.zeros((0, 3), LD), np.zeros(0, np.float32), np.zeros(0), np.zeros(0), [])
    return Assembly(np.concatenate(xyz), np.concatenate(c), np.concatenate(pa), np.concatenate(ta), segs)


def filtered(raw_xyzc, leaf):
    """pcl::VoxelGrid over an assembled (n, 4) float32 cloud: pre_reference.voxelgrid's output"""
    return pr.voxelgrid(np.asarray(raw_xyzc, np.float32), np.float32(leaf))


def quaternion_of(pose):
    """x, y, z, w (float64) of the rotation, by the textbook trace formula on the longdouble matrix: what a test hands to rgc_transform_cloud as the
    second witness needs only to be A unit quaternion of this rotation; bit-equality is asked against the library's own quaternion, which a test
    obtains from the library (rgc_ypr2R) and not from here"""
    R = rotation(pose)
    w = np.sqrt(max(LD(0), 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-6:
        return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w], np.float64)
    x = np.sqrt(max(LD(0), 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    return np.array([x, (R[0, 1] + R[1, 0]) / (4 * x), (R[0, 2] + R[2, 0]) / (4 * x), (R[2, 1] - R[1, 2]) / (4 * x)], np.float64)
