// rgc::KeyframeStore::optimizePoseGraph / rgc::makeLoop (rgc-slam_amd/cpp/keyframe_store.hpp) over the C-ABI's rgc_pgo_*: a store of key poses read
// from a file, one loop edge made from a drift matrix, the pose graph optimised without and with write-back.  Prints what tests/test_pgo_cpp.py
// compares with the Python class on the same input.
//   test_pose_graph poses.bin     (int32 n, then n x 6 float32 {x, y, z, roll, pitch, yaw})
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rgc-slam_amd/cpp/keyframe_store.hpp"

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s poses.bin\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  int n = 0;
  if (!f || std::fread(&n, 4, 1, f) != 1 || n < 3) return 2;
  std::vector<float> raw((std::size_t)n * 6);
  if (std::fread(raw.data(), 4, raw.size(), f) != raw.size()) return 2;
  std::fclose(f);
  try {
    rgc::KeyframeStore store(0);
    std::vector<int> ids;
    std::vector<rgc_kf_pose> poses;
    for (int i = 0; i < n; i++) {
      rgc_kf_pose p;
      std::memcpy(&p, &raw[(std::size_t)i * 6], sizeof(p));
      poses.push_back(p);
      ids.push_back(10 + 2 * i);
      store.push(ids.back(), p, nullptr, 0, nullptr, 0, nullptr, 0, 16);
    }
    const float T[16] = {1, 0, 0, 0.3f, 0, 1, 0, -0.2f, 0, 0, 1, 0.05f, 0, 0, 0, 1};
    std::vector<rgc_pgo_loop> loops{rgc::makeLoop(poses[n - 1], poses[1], T, ids[n - 1], ids[1])};
    std::printf("loop %d %d %.17g %.17g %.17g %.17g %.17g %.17g\n", loops[0].key_curr, loops[0].key_loop, loops[0].t_loop_curr[0], loops[0].t_loop_curr[1],
                loops[0].t_loop_curr[2], loops[0].yaw_loop_curr_deg, loops[0].pitch_loop_deg, loops[0].roll_loop_deg);
    const unsigned long long rev = store.info().revision;
    std::vector<rgc_kf_pose> out;
    rgc_pgo_report rep = store.optimizePoseGraph(ids, loops, false, &out);
    if (store.info().revision != rev) { std::fprintf(stderr, "apply = false changed the store\n"); return 1; }
    rep = store.optimizePoseGraph(ids, loops, true, &out);
    if (store.info().revision != rev + 1) { std::fprintf(stderr, "apply = true did not bump the revision once\n"); return 1; }
    std::printf("report %d %d %d %d %d %d %d %d %.17g %.17g\n", rep.status, rep.n_nodes, rep.n_loops_used, rep.fixed_id, rep.iterations, rep.successful, rep.stop,
                (int)rep.accepted_mask, rep.initial_cost, rep.final_cost);
    for (int i = 0; i < n; i++) std::printf("pose %.9g %.9g %.9g %.9g %.9g %.9g\n", out[i].x, out[i].y, out[i].z, out[i].roll, out[i].pitch, out[i].yaw);
    rgc_pgo_report none = store.optimizePoseGraph(ids, std::vector<rgc_pgo_loop>());
    std::printf("no_loop %d\n", none.status);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
