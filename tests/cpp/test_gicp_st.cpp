// rgc::FastGICPSingleThreadHip (rgc-slam_amd/cpp/fast_gicp_hip.hpp) used the way a caller of fast_gicp::FastGICPSingleThread would: pcl-style clouds,
// the reference's setters, align -- also through a FastGICPHip reference, as the reference class is used through FastGICP's.  Compiled -Wall -Wextra
// -Werror by tests/test_gicp_st_api.py (no GPU needed for that); run on a GPU it registers a shifted copy of a three-plane cloud and returns 0 when the
// solve converges onto the shift, a second linearisation at the same pose searches fewer points than there are, the first one after a reset searches
// them all, and the frozen cost equals the linearised one (tests/test_gpu_gicp_st.py holds the library to the numpy reference).
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

static bool solve(rgc::FastGICPHip& reg) {   // the derived class behind the base's interface
  reg.align();
  const rgc::FastGICPHip::Matrix4f& T = reg.getFinalTransformation();
  std::printf("t = %.4f %.4f %.4f, %d iterations, converged %d, fitness %.6f\n", T[3], T[7], T[11], reg.iterations(), (int)reg.hasConverged(), reg.getFitnessScore());
  return reg.hasConverged() && !reg.lmFailed() && std::fabs(T[3] - 0.10f) <= 0.01f && std::fabs(T[7] + 0.05f) <= 0.01f && std::fabs(T[11] - 0.03f) <= 0.01f;
}

int main() {
  try {
    rgc::FastGICPSingleThreadHip st(0);
    st.setCorrespondenceRandomness(20);
    st.setInputTarget(make(0.f, 0.f, 0.f));
    st.setInputSource(make(-0.10f, 0.05f, -0.03f));
    int bad = solve(st) ? 0 : 1;
    const rgc::FastGICPHip::Matrix4d I = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    rgc::FastGICPHip::Matrix6d H;
    rgc::FastGICPHip::Vector6d b;
    st.reset();
    const double y0 = st.linearize(I, &H, &b), y1 = st.compute_error(I);
    const int first = st.numSearched(), all = st.numCorrespondences();
    st.linearize(I);
    const int again = st.numSearched();
    std::vector<int> idx, searched;
    std::vector<float> sq, sq2;
    st.getCorrespondences(idx, sq, sq2, searched);
    int counted = 0, ordered = 0;
    for (size_t i = 0; i < idx.size(); i++) { counted += searched[i]; ordered += sq[i] <= sq2[i] ? 1 : 0; }
    std::printf("cost %.6f / %.6f, pairs %d of 20000, searched %d then %d (%d counted), key1 <= key2 on %d\n", y0, y1, all, first, again, counted, ordered);
    if (first != 20000 || all != 20000 || again >= first || counted != again || ordered != 20000) bad++;
    return bad == 0 && y0 == y1 ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
}
