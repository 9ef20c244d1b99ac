// rgc::KeyframeStore (rgc-slam_amd/cpp/keyframe_store.hpp) used the way the mapping node would: pcl-style clouds pushed with PointXYZIRPYT-like
// poses, a pose-graph correction, the three assemblies.  Compiled -Wall -Wextra -Werror by tests/test_kf_reference.py (no GPU needed for that);
// run on a GPU it prints the counts and returns 0 when the concatenation has the stored number of points.
#include <cstdio>
#include <memory>
#include <vector>

#include "../../rgc-slam_amd/cpp/keyframe_store.hpp"

struct Point { float x, y, z, data3, intensity, normal_x, pad[2]; };   // a 32-byte point, x y z c first
struct Cloud { std::vector<Point> points; };
struct Pose6D { float x, y, z, intensity, roll, pitch, yaw; double time; };

static std::shared_ptr<Cloud> make(int n, float z) {
  auto c = std::make_shared<Cloud>();
  for (int i = 0; i < n; i++) c->points.push_back(Point{0.1f * (float)i, 0.05f * (float)(i % 7), z, 1.0f, 0.f, 0.f, {0.f, 0.f}});
  return c;
}

int main() {
  try {
    rgc::KeyframeStore store(0);
    std::vector<int> ids;
    for (int k = 0; k < 5; k++) {
      const Pose6D p{(float)k, 0.5f * (float)k, 0.f, (float)k, 0.01f, -0.02f, 0.3f * (float)k, 0.0};
      store.push(k, rgc::KeyframeStore::pose(p), make(40 + k, 0.f), make(300, 1.f), std::shared_ptr<Cloud>());
      ids.push_back(k);
    }
    store.setPoses({1, 3}, {rgc_kf_pose{1.f, 1.f, 0.f, 0.f, 0.f, 0.5f}, rgc_kf_pose{3.f, 1.f, 0.f, 0.f, 0.f, 1.5f}});
    const rgc_kf_info info = store.info();
    const std::vector<float> raw = store.assemble(ids, rgc::KeyframeStore::CORNER | rgc::KeyframeStore::SURF);
    rgc::DeviceCloud ds = store.assembleDevice(ids, rgc::KeyframeStore::SURF, 0.4f);
    std::printf("keyframes %d corner %lld surf %lld raw %zu filtered %d of %d\n", info.n_keyframes, info.n_points[0], info.n_points[1], raw.size() / 4,
                ds.size(), ds.rawSize());
    return raw.size() / 4 == (size_t)(info.n_points[0] + info.n_points[1]) && ds.size() > 0 && ds.size() <= ds.rawSize() ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
}
