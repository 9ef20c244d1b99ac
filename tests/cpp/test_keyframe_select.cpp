// rgc::KeyframeStore::travel / selectSurrounding / selectGlobal / detectLoop and rgc::uniformSampling (rgc-slam_amd/cpp/keyframe_store.hpp) over the
// C-ABI's rgc_kf_* and rgc_uniform_sampling: a store of key poses read from a file, four points pushed per keyframe.  Prints what
// tests/test_kf_select_cpp.py compares with the Python layer on the same input.
//   test_keyframe_select poses.bin     (int32 n, then n x 6 float32 {x, y, z, roll, pitch, yaw}; ids = positions)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rgc-slam_amd/cpp/keyframe_store.hpp"

static void print_ids(const char* tag, const std::vector<int>& v) {
  std::printf("%s", tag);
  for (int i : v) std::printf(" %d", i);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s poses.bin\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  int n = 0;
  if (!f || std::fread(&n, 4, 1, f) != 1 || n < 1) return 2;
  std::vector<float> raw((std::size_t)n * 6);
  if (std::fread(raw.data(), 4, raw.size(), f) != raw.size()) return 2;
  std::fclose(f);
  try {
    rgc::KeyframeStore store(0);
    std::vector<int> ids;
    for (int i = 0; i < n; i++) {
      rgc_kf_pose p;
      std::memcpy(&p, &raw[(std::size_t)i * 6], sizeof(p));
      const float pts[16] = {0.1f, 0.2f, 0.3f, 1.f, -0.1f, 0.2f, 0.f, 2.f, 0.3f, -0.2f, 0.1f, 3.f, 0.f, 0.f, 0.5f, 4.f};
      store.push(i, p, pts, 4, pts, 2, nullptr, 0, 16);
      ids.push_back(i);
    }
    std::vector<float> dist, ang;
    store.travel(ids, &dist, &ang);
    std::printf("travel %.9g %.9g\n", dist.back(), ang.back());
    int n_in = 0;
    print_ids("surrounding", store.selectSurrounding(raw[(std::size_t)(n - 1) * 6], raw[(std::size_t)(n - 1) * 6 + 1], raw[(std::size_t)(n - 1) * 6 + 2], 15.f, 0.3f, &n_in));
    std::printf("in_radius %d\n", n_in);
    print_ids("global", store.selectGlobal(0.5f));
    const rgc::LoopDetection d = store.detectLoop();
    std::printf("loop %d %d %d %.9g %d\n", d.candidate.found, d.candidate.latest_id, d.candidate.closest_id, d.candidate.search_radius, d.candidate.n_in_radius);
    print_ids("history", d.history_ids);
    rgc_kf_loop_params prm;
    rgc_default_kf_loop_params(&prm);
    prm.min_key_id = 0;
    prm.history_search_num = 2;
    const rgc::LoopDetection d2 = store.detectLoop(&prm);
    std::printf("loop2 %d %d %d\n", d2.candidate.found, d2.candidate.closest_id, (int)d2.history_ids.size());
    std::vector<float> xyz;
    for (int i = 0; i < n; i++) for (int a = 0; a < 3; a++) xyz.push_back(raw[(std::size_t)i * 6 + a]);
    std::vector<int> index;
    const std::vector<float> us = rgc::uniformSampling(store.context(), xyz.data(), n, 12, 0.5f, &index);
    print_ids("sampling", index);
    if (us.size() != index.size() * 4) return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
