// FastVGICPCuda::setNeighborSearchMethod(method, radius) on the C++ adaptor (fast_vgicp_cuda.hpp:60) with the reference's signature.  Clouds from raw
// float files written by the Python test; prints what the test compares: the linearisation and the solve under DIRECT_RADIUS 2.0, the selection read
// back, and the statuses of the setters (a refused radius is remembered, not thrown, and stays pending until a valid one replaces it).
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
  const double I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  try {
    rgc::FastVGICPHip vgicp;
    Cloud aligned;
    int ok = 0;
    double r = -7.0;
    vgicp.setResolution(1.0);
    vgicp.setMaximumIterations(25);
    vgicp.setTransformationEpsilon(1e-6);
    ok += vgicp.getNeighborSearchMethod(&r) == rgc::NeighborSearchMethod::DIRECT1 && r == 0.0;       // a new context: DIRECT1, radius 0
    vgicp.setNeighborSearchMethod(rgc::NeighborSearchMethod::DIRECT_RADIUS, 2.0);
    ok += vgicp.lastSetterStatus() == RGC_OK;
    vgicp.setMaximumIterations(25);                                                                   // pushes the whole block: the method stays
    ok += vgicp.getNeighborSearchMethod(&r) == rgc::NeighborSearchMethod::DIRECT_RADIUS && r == 2.0;
    vgicp.setInputTarget(target);
    vgicp.setInputSource(source);
    double H[36], b[6];
    const double cost = vgicp.linearize(I16, H, b);
    printf("lin %.17g", cost);
    for (int a = 0; a < 36; a++) printf(" %.17g", H[a]);
    for (int a = 0; a < 6; a++) printf(" %.17g", b[a]);
    printf("\n");
    vgicp.align(aligned, T0);
    Mat4 T = vgicp.getFinalTransformation<Mat4>();
    printf("T");
    for (int i = 0; i < 16; i++) printf(" %.9g", T.m[i]);
    printf("\nconverged %d iterations %d\n", (int)vgicp.hasConverged(), vgicp.iterations());
    vgicp.setNeighborSearchMethod(rgc::NeighborSearchMethod::DIRECT_RADIUS, 5.0);                    // 515 offsets: refused, remembered, pending
    ok += vgicp.lastSetterStatus() == RGC_ERR_INVALID;
    ok += vgicp.getNeighborSearchMethod(&r) == rgc::NeighborSearchMethod::DIRECT_RADIUS && r == 2.0;  // the context as it was
    try { vgicp.align(aligned, T0); } catch (const std::exception&) { ok++; }                         // ... so the next computation throws
    vgicp.setNeighborSearchMethod(rgc::NeighborSearchMethod::DIRECT7);                                // the default radius of -1 is ignored
    ok += vgicp.lastSetterStatus() == RGC_OK;
    ok += vgicp.getNeighborSearchMethod(&r) == rgc::NeighborSearchMethod::DIRECT7 && r == 2.0;       // the stored radius stays
    vgicp.align(aligned, T0);
    ok += vgicp.hasConverged();
    printf("setters %d\n", ok);
  } catch (const std::exception& e) {
    printf("EXCEPTION %s\n", e.what());
    return 1;
  }
  return 0;
}
