// rgc::FastGICPMultiPointsHip (rgc-slam_amd/cpp/fast_gicp_hip.hpp) used the way a caller of fast_gicp::FastGICPMultiPoints would: pcl-style clouds, the
// reference's setters, align.  Compiled -Wall -Wextra -Werror by tests/test_gicp_mp_reference.py (no GPU needed for that); run on a GPU it registers a
// shifted copy of a three-plane cloud and returns 0 when the solve converges onto the shift, the merged list and the CSR rows of the last linearisation
// agree with each other and with the two counts, and a smaller radius finds fewer neighbours (tests/test_gpu_gicp_mp.py holds the library to the numpy
// reference).
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
    rgc::FastGICPMultiPointsHip mp(0);
    mp.setNumThreads(4);
    mp.setCorrespondenceRandomness(20);
    mp.setRegularizationMethod(RGC_REG_PLANE);
    mp.setNeighborSearchRadius(0.5);
    mp.setRotationEpsilon(1e-5);
    mp.setTransformationEpsilon(1e-5);
    mp.setMaximumIterations(64);
    mp.setInputTarget(make(0.f, 0.f, 0.f));
    mp.setInputSource(make(-0.10f, 0.05f, -0.03f));
    int bad = 0;
    mp.align();
    const rgc::FastGICPMultiPointsHip::Matrix4f& T = mp.getFinalTransformation();
    std::printf("t = %.4f %.4f %.4f, %d iterations, converged %d, failed %d, fitness %.6f\n", T[3], T[7], T[11], mp.iterations(), (int)mp.hasConverged(), (int)mp.failed(),
                mp.getFitnessScore());
    if (!mp.hasConverged() || mp.failed()) bad++;
    if (std::fabs(T[3] - 0.10f) > 0.01f || std::fabs(T[7] + 0.05f) > 0.01f || std::fabs(T[11] - 0.03f) > 0.01f) bad++;
    const rgc::FastGICPMultiPointsHip::Matrix4d I = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    rgc::FastGICPMultiPointsHip::Matrix6d H;
    rgc::FastGICPMultiPointsHip::Vector6d b;
    const double y0 = mp.linearize(I, &H, &b), y1 = mp.linearize(I);
    const int points = mp.numCorrespondences();
    const long long pairs = mp.numPairs();
    std::vector<int> count, offsets, idx;
    std::vector<double> sw, mean3, cov6;
    std::vector<float> sq;
    mp.merged(count, sw, mean3, cov6);
    mp.neighbors(offsets, idx, sq);
    long long sum = 0;
    int with = 0, rows_ok = 1;
    for (size_t i = 0; i < count.size(); i++) {
      sum += count[i];
      with += count[i] > 0 ? 1 : 0;
      if (offsets[i + 1] - offsets[i] != count[i]) rows_ok = 0;
      if ((count[i] > 0) != (sw[i] > 0.0)) rows_ok = 0;
    }
    for (size_t k = 0; k < idx.size(); k++)
      if (idx[k] < 0 || idx[k] >= 20000 || !(sq[k] < 0.25f)) rows_ok = 0;
    std::printf("cost %.6f / %.6f, %d of 20000 points with a neighbour, %lld neighbours (%lld counted, %zu listed)\n", y0, y1, points, pairs, sum, idx.size());
    if (with != points || sum != pairs || (long long)idx.size() != pairs || !rows_ok || points < 15000) bad++;
    mp.setNeighborSearchRadius(0.1);
    mp.linearize(I);
    if (mp.numPairs() >= pairs || mp.getNeighborSearchRadius() != 0.1) bad++;
    return bad == 0 && y0 == y1 ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
}
