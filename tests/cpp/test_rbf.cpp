// FastVGICPCuda's pair of setters on the C++ adaptor (fast_vgicp_cuda.hpp:58,61): setNearestNeighborSearchMethod / setKernelWidth with the reference's
// signatures.  Clouds from raw float files written by the Python test; prints what the test compares: the RBF covariances of the first target points,
// the solve under RBF, and the statuses of the setters.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rgc-slam_amd/cpp/fast_vgicp_hip.hpp"

struct PointXYZ { float x, y, z, pad; };
struct Cloud { std::vector<PointXYZ> points; size_t size() const { return points.size(); } };
struct Mat4 { float m[16]; float& operator()(int r, int c) { return m[r * 4 + c]; } float operator()(int r, int c) const { return m[r * 4 + c]; } };

static Cloud* load(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  int n = 0;
  if (fread(&n, 4, 1, f) != 1) exit(2);
  std::vector<float> xyz((size_t)n * 3);
  if (fread(xyz.data(), 4, xyz.size(), f) != xyz.size()) exit(2);
  fclose(f);
  Cloud* c = new Cloud;
  c->points.resize(n);
  for (int i = 0; i < n; i++) c->points[i] = PointXYZ{xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], 1.f};
  return c;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  Cloud* target = load(argv[1]);
  Cloud* source = load(argv[2]);
  Mat4 T0{};
  for (int i = 0; i < 4; i++) T0(i, i) = 1.f;
  try {
    rgc::FastVGICPHip vgicp;
    Cloud aligned;
    vgicp.setResolution(1.0);
    vgicp.setRegularizationMethod(rgc::RegularizationMethod::MIN_EIG);
    int ok = 0;
    vgicp.setNearestNeighborSearchMethod(rgc::NearestNeighborMethod::GPU_RBF_KERNEL);
    ok += vgicp.lastSetterStatus() == RGC_OK;
    vgicp.setKernelWidth(0.5, 3.0);
    ok += vgicp.lastSetterStatus() == RGC_OK;
    vgicp.setInputTarget(target);
    vgicp.setInputSource(source);
    const std::vector<double> cov = vgicp.getTargetCovariances();
    for (int i = 0; i < 4; i++) {
      printf("cov %d", i);
      for (int a = 0; a < 9; a++) printf(" %.17g", cov[(size_t)i * 9 + a]);
      printf("\n");
    }
    vgicp.align(aligned, T0);
    Mat4 T = vgicp.getFinalTransformation<Mat4>();
    printf("T");
    for (int i = 0; i < 16; i++) printf(" %.9g", T.m[i]);
    printf("\nconverged %d\n", (int)vgicp.hasConverged());
    vgicp.setKernelWidth(0.25);                                     // max_dist defaults to -1: 5 * kernel_width
    ok += vgicp.lastSetterStatus() == RGC_OK;
    try { vgicp.align(aligned, T0); } catch (const std::exception&) { ok++; }   // another kernel under RBF dropped the clouds
    vgicp.setKernelWidth(0.0);
    ok += vgicp.lastSetterStatus() == RGC_ERR_INVALID;             // remembered, not thrown: the reference's setters cannot fail
    vgicp.setKernelWidth(0.5, 3.0);
    vgicp.setNearestNeighborSearchMethod(rgc::NearestNeighborMethod::GPU_BRUTEFORCE);
    vgicp.setNearestNeighborSearchMethod(rgc::NearestNeighborMethod::CPU_PARALLEL_KDTREE);   // both the exact kNN: the second call changes nothing
    ok += vgicp.lastSetterStatus() == RGC_OK;
    vgicp.setInputTarget(target);
    vgicp.setInputSource(source);
    const std::vector<double> knn = vgicp.getTargetCovariances();
    int differs = 0;
    for (int a = 0; a < 9; a++) differs |= knn[a] != cov[a];
    printf("setters %d differs %d\n", ok, differs);
  } catch (const std::exception& e) {
    printf("EXCEPTION %s\n", e.what());
    return 1;
  }
  return 0;
}
