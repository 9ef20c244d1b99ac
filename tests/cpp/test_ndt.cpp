// rgc::NDTHip (rgc-slam_amd/cpp/ndt_hip.hpp) used the way a caller of fast_gicp::NDTCuda would: pcl-style clouds, the reference's setters, align.
// Compiled -Wall -Wextra -Werror by tests/test_ndt_reference.py (no GPU needed for that); run on a GPU it registers a shifted copy of a
// three-plane cloud in both distance modes and returns 0 when both solves converge towards the shift (how close the minimum of a toy cloud lies to it is
// not this program's business: tests/test_gpu_ndt.py holds the library to the numpy reference).
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../rgc-slam_amd/cpp/ndt_hip.hpp"

struct Point { float x, y, z, intensity; };
struct Cloud { std::vector<Point> points; };

static std::shared_ptr<Cloud> make(float dx, float dy, float dz) {
  auto c = std::make_shared<Cloud>();
  unsigned s = 12345u;
  auto rnd = [&s]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
  for (int i = 0; i < 20000; i++) {
    const float u = 20.f * rnd() - 10.f, v = 20.f * rnd() - 10.f, n = 0.02f * (rnd() - 0.5f);
    if (i % 3 == 0) c->points.push_back(Point{u + dx, v + dy, n + dz, 0.f});                 // floor
    else if (i % 3 == 1) c->points.push_back(Point{u + dx, 4.f + n + dy, 1.5f + 0.15f * v + dz, 0.f});  // wall
    else c->points.push_back(Point{-3.f + n + dx, u + dy, 1.5f + 0.15f * v + dz, 0.f});                 // another
  }
  return c;
}

int main() {
  try {
    rgc::NDTHip ndt(0);
    ndt.setResolution(1.0);
    ndt.setInputTarget(make(0.f, 0.f, 0.f));
    ndt.setInputSource(make(-0.10f, 0.05f, -0.03f));
    int bad = 0;
    for (int mode : {RGC_NDT_D2D, RGC_NDT_P2D}) {
      ndt.setDistanceMode(mode);
      ndt.setNeighborSearchMethod(RGC_NDT_DIRECT7);
      ndt.align();
      const rgc::NDTHip::Matrix4f& T = ndt.getFinalTransformation();
      std::printf("mode %d: t = %.4f %.4f %.4f, %d iterations, converged %d\n", mode, T[3], T[7], T[11], ndt.iterations(), (int)ndt.hasConverged());
      if (!ndt.hasConverged() || ndt.lmFailed() || !(T[3] * 0.10f - T[7] * 0.05f + T[11] * 0.03f > 0.f)) bad++;
    }
    ndt.setNeighborSearchMethod(RGC_NDT_DIRECT_RADIUS, 1.5);
    const rgc::NDTHip::Matrix4d I = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    rgc::NDTHip::Matrix6d H;
    rgc::NDTHip::Vector6d b;
    const double y0 = ndt.linearize(I, &H, &b), y1 = ndt.compute_error(I);
    std::printf("radius 1.5: cost %.6f / %.6f\n", y0, y1);
    return bad == 0 && y0 == y1 ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
}
