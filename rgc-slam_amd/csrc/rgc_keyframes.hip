// rgc_keyframes.hip -- gfx950 kernel of the mapping node's keyframe store (f5): the body-frame clouds of a SELECTION of keyframes
// re-expressed by their current key poses and concatenated, in one launch.  Reference: transformPointCloud(cloud, &pose6D) per selected
// keyframe and `+=` into one cloud (src/RGC_mapping.cpp:2567-2612 called from :1591-1592, 2186-2214, 2516-2526); citations are
// relative to rgc_slam/ of the reference (ROBOT-WSC/RGC-SLAM).
#include "rgc_kernels.h"

namespace rgck {

// One SEGMENT of the table = one (keyframe, kind) of the selection: n stored points at src, written to out[out0 .. out0 + n).  The
// launch's workgroups are dealt to the segments through blk0 (first workgroup of segment s; blk0[nseg] = the grid size): a workgroup
// never straddles two segments, so the segment -- found by a binary search every lane runs on blockIdx.x alone -- and with it the
// pose are wave-uniform: the table is read through scalar loads into scalar registers, once per wave.  Per point: one 16-byte load, the
// fp64 arithmetic of k_transform_q (q * p + t, Eigen's quaternion-vector product, stored fp32, fourth float copied: same expressions in
// the same order, so the same bits), one 16-byte store; consecutive lanes touch consecutive points on both sides.
__global__ void __launch_bounds__(kKfBlock) k_kf_assemble(const KfSegment* __restrict__ seg, const int* __restrict__ blk0, int nseg, float4* __restrict__ out) {
  const int b = blockIdx.x;
  int lo = 0, hi = nseg;  // blk0[lo] <= b < blk0[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (blk0[mid] <= b) lo = mid; else hi = mid;
  }
  const KfSegment& S = seg[lo];
  const int i = (b - blk0[lo]) * kKfBlock + (int)threadIdx.x;
  if (i >= S.n) return;
  const Quat q = S.q;
  const float4 p = S.src[i];
  const double vx = (double)p.x, vy = (double)p.y, vz = (double)p.z;
  double ux = q.y * vz - q.z * vy, uy = q.z * vx - q.x * vz, uz = q.x * vy - q.y * vx;
  ux += ux; uy += uy; uz += uz;
  float4 o;
  o.x = (float)(vx + q.w * ux + (q.y * uz - q.z * uy) + S.t[0]);
  o.y = (float)(vy + q.w * uy + (q.z * ux - q.x * uz) + S.t[1]);
  o.z = (float)(vz + q.w * uz + (q.x * uy - q.y * ux) + S.t[2]);
  o.w = p.w;
  out[(size_t)S.out0 + (size_t)i] = o;
}

void kf_assemble(hipStream_t s, const KfSegment* seg, const int* blk0, int nseg, int nblocks, float4* out) {
  if (nseg > 0 && nblocks > 0) hipLaunchKernelGGL(k_kf_assemble, dim3(nblocks), dim3(kKfBlock), 0, s, seg, blk0, nseg, out);
}

}  // namespace rgck
