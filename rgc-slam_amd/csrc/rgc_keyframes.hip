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

// ---- the mapping node's keyframe selections (src/RGC_mapping.cpp:1525-1548, 2141-2225, 2493-2505) over the device mirror of the key positions ----
// One lane per store position p: d2 = (dx*dx + dy*dy) + dz*dz in fp32, uncontracted (flann::L2_Simple<float> [3P-memory]); inside = d2 < r2, strict.
//   flag[p] (nullable) = inside, the input of the ordered compaction;  small[0] += the number inside (one add per wave);
//   loop != 0: a position qualifies when it is inside, |travel[p] - travel_last| > thr and ids[p] >= min_id; the two words at small + 2 take the
//   64-bit minimum of (bits of d2) << 32 | p -- d2 >= 0, so bit order is value order, and a minimum is the same in any arrival order.
__global__ void __launch_bounds__(256) k_kf_gate(const float4* __restrict__ pos, const float* __restrict__ travel, const int* __restrict__ ids, int n, float qx,
                                                 float qy, float qz, float r2, int loop, float travel_last, float thr, int min_id, int* __restrict__ flag,
                                                 unsigned* small) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  bool inside = false;
  unsigned long long key = ~0ull;
  if (p < n) {
    const float4 c = pos[p];
    const float dx = c.x - qx, dy = c.y - qy, dz = c.z - qz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    inside = d2 < r2;
    if (flag) flag[p] = inside ? 1 : 0;
    if (loop && inside && fabsf(travel[p] - travel_last) > thr && ids[p] >= min_id) key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)p;
  }
  const unsigned long long m = __ballot(inside);
  const int lane = threadIdx.x & 63;
  if (m && lane == 0) atomicAdd(&small[0], (unsigned)__popcll(m));
  if (loop) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(key, o);
      key = other < key ? other : key;
    }
    if (lane == 0 && key != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(small + 2), key);
  }
}
// the in-radius positions in ascending store position: out[scan[p]] = {x, y, z, position} of every flagged p
__global__ void k_kf_compact(const float4* __restrict__ pos, const int* __restrict__ flag, const int* __restrict__ scan, int n, float4* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n && flag[p]) out[scan[p]] = pos[p];
}

void kf_gate(hipStream_t s, const float4* pos, const float* travel, const int* ids, int n, const float q[3], float r2, int loop, float travel_last, float thr,
             int min_id, int* flag, unsigned* small) {
  if (n > 0) hipLaunchKernelGGL(k_kf_gate, dim3((n + 255) / 256), dim3(256), 0, s, pos, travel, ids, n, q[0], q[1], q[2], r2, loop, travel_last, thr, min_id, flag, small);
}
void kf_compact(hipStream_t s, const float4* pos, const int* flag, const int* scan, int n, float4* out) {
  if (n > 0) hipLaunchKernelGGL(k_kf_compact, dim3((n + 255) / 256), dim3(256), 0, s, pos, flag, scan, n, out);
}

}  // namespace rgck
