// rgc::KdTreeHip (rgc-slam_amd/cpp/kdtree_hip.hpp) used the way a caller of pcl::KdTreeFLANN would: pcl-style clouds, setInputCloud, nearestKSearch and
// radiusSearch of one point, their batched forms over a whole cloud, setSortedResults.  Compiled -Wall -Wextra -Werror by tests/test_search_api.py (no GPU
// needed for that); tests/test_gpu_cpp_kdtree.py runs it on a GPU with two files of float32 x, y, z rows (the indexed cloud, the queries) and compares the
// rows it prints -- indices and the keys' bit patterns -- with the numpy reference.  Line format: <tag> <query> <count> then count pairs "index keybits";
// tags: K batched 5-NN, k single-point 7-NN (first 8 queries), R batched sorted radius 0.125, r single-point radius 0.125 with max_nn 3 (first 8), U batched
// unsorted radius 0.125.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../rgc-slam_amd/cpp/kdtree_hip.hpp"

struct Point { float x, y, z, intensity; };
struct Cloud { std::vector<Point> points; };

static std::shared_ptr<Cloud> read_cloud(const char* path) {
  auto c = std::make_shared<Cloud>();
  std::FILE* f = std::fopen(path, "rb");
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  float v[3];
  while (std::fread(v, sizeof(float), 3, f) == 3) c->points.push_back(Point{v[0], v[1], v[2], 0.f});
  std::fclose(f);
  return c;
}
static unsigned bits(float v) {
  unsigned u;
  std::memcpy(&u, &v, sizeof(u));
  return u;
}
static void print_row(const char* tag, size_t q, const int* idx, const float* sq, size_t n) {
  std::printf("%s %zu %zu", tag, q, n);
  for (size_t j = 0; j < n; j++) std::printf(" %d %u", idx[j], bits(sq[j]));
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: test_kdtree <cloud.f32> <queries.f32>\n");
    return 2;
  }
  try {
    const auto cloud = read_cloud(argv[1]), queries = read_cloud(argv[2]);
    rgc::KdTreeHip tree(0);
    tree.setInputCloud(cloud);
    const size_t nq = queries->points.size(), few = nq < 8 ? nq : 8;
    std::vector<int> idx, off;
    std::vector<float> sq;
    tree.nearestKSearch(queries, 5, idx, sq);
    for (size_t i = 0; i < nq; i++) print_row("K", i, &idx[5 * i], &sq[5 * i], 5);
    for (size_t i = 0; i < few; i++) {
      const int found = tree.nearestKSearch(queries->points[i], 7, idx, sq);
      if ((size_t)found != idx.size()) return 1;
      print_row("k", i, idx.data(), sq.data(), idx.size());
    }
    long long total = tree.radiusSearch(queries, 0.125, off, idx, sq);
    if (total != (long long)idx.size() || off.size() != nq + 1 || off[nq] != total) return 1;
    for (size_t i = 0; i < nq; i++) print_row("R", i, idx.data() + off[i], sq.data() + off[i], (size_t)(off[i + 1] - off[i]));
    for (size_t i = 0; i < few; i++) {
      const int found = tree.radiusSearch(queries->points[i], 0.125, idx, sq, 3);
      if ((size_t)found != idx.size() || found > 3) return 1;
      print_row("r", i, idx.data(), sq.data(), idx.size());
    }
    tree.setSortedResults(false);
    total = tree.radiusSearch(queries, 0.125, off, idx, sq);
    for (size_t i = 0; i < nq; i++) print_row("U", i, idx.data() + off[i], sq.data() + off[i], (size_t)(off[i + 1] - off[i]));
    const rgc_search_info s = tree.info();
    std::fprintf(stderr, "%d points indexed, cell %g, %lld cells; last call looked at %lld candidates\n", s.n, s.cell, s.cells, s.candidates);
    return s.n == (int)cloud->points.size() && total == off[nq] ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
}
