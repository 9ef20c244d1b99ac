// rgc::FastGICPHip (rgc-slam_amd/cpp/fast_gicp_hip.hpp) used the way a caller of fast_gicp::FastGICP would: pcl-style clouds, the reference's setters,
// align.  Compiled -Wall -Wextra -Werror by tests/test_gicp_reference.py (no GPU needed for that); run on a GPU it registers a shifted copy of a
// three-plane cloud and returns 0 when the solve converges onto the shift, the frozen cost equals the linearised one at the same pose, every source
// point has a pair by default and fewer have one under a small maximum distance (tests/test_gpu_gicp.py holds the library to the numpy reference).
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../rgc-slam_amd/cpp/fast_gicp_hip.hpp"

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
    rgc::FastGICPHip gicp(0);
    gicp.setCorrespondenceRandomness(20);
    gicp.setInputTarget(make(0.f, 0.f, 0.f));
    gicp.setInputSource(make(-0.10f, 0.05f, -0.03f));
    int bad = 0;
    gicp.align();
    const rgc::FastGICPHip::Matrix4f& T = gicp.getFinalTransformation();
    std::printf("t = %.4f %.4f %.4f, %d iterations, converged %d, fitness %.6f\n", T[3], T[7], T[11], gicp.iterations(), (int)gicp.hasConverged(), gicp.getFitnessScore());
    if (!gicp.hasConverged() || gicp.lmFailed()) bad++;
    if (std::fabs(T[3] - 0.10f) > 0.01f || std::fabs(T[7] + 0.05f) > 0.01f || std::fabs(T[11] - 0.03f) > 0.01f) bad++;
    const rgc::FastGICPHip::Matrix4d I = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    rgc::FastGICPHip::Matrix6d H;
    rgc::FastGICPHip::Vector6d b;
    const double y0 = gicp.linearize(I, &H, &b), y1 = gicp.compute_error(I);
    const int all = gicp.numCorrespondences();
    gicp.setMaxCorrespondenceDistance(0.05);
    gicp.linearize(I);
    std::vector<int> idx;
    std::vector<float> sq;
    gicp.getCorrespondences(idx, sq);
    int kept = 0;
    for (size_t i = 0; i < idx.size(); i++) kept += idx[i] >= 0 ? 1 : 0;
    std::printf("cost %.6f / %.6f, pairs %d of 20000, %d within 0.05 m (%d counted)\n", y0, y1, all, gicp.numCorrespondences(), kept);
    if (all != 20000 || kept != gicp.numCorrespondences() || kept >= all) bad++;
    return bad == 0 && y0 == y1 ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
}
