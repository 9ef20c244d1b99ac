// rgc::EuclideanClusterExtractionHip (rgc-slam_amd/cpp/segmentation_hip.hpp) used the way a caller of pcl::EuclideanClusterExtraction would: a pcl-style
// cloud, setInputCloud, the three setters, extract(clusters).  Compiled -Wall -Wextra -Werror by tests/test_cluster_api.py (no GPU needed for that);
// tests/test_gpu_cpp_segmentation.py runs it on a GPU with a file of float32 x, y, z rows and compares the lines it prints with the numpy reference for
// equality.  usage: test_segmentation <cloud.f32> <tolerance> <min_size> <max_size>
// Line format: <tag> <count> then the values; tags: M the number of clusters (one value), C one line per cluster in rank order (its members), L the labels.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../rgc-slam_amd/cpp/segmentation_hip.hpp"

struct Point { float x, y, z, intensity; };
struct Cloud { std::vector<Point> points; };

static std::shared_ptr<Cloud> read_cloud(const char* path) {
  auto c = std::make_shared<Cloud>();
  std::FILE* f = std::fopen(path, "rb");
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  float v[3];
  while (std::fread(v, sizeof(float), 3, f) == 3) c->points.push_back(Point{v[0], v[1], v[2], (float)c->points.size()});
  std::fclose(f);
  return c;
}
static void print_row(const char* tag, const std::vector<int>& v) {
  std::printf("%s %zu", tag, v.size());
  for (int x : v) std::printf(" %d", x);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: test_segmentation <cloud.f32> <tolerance> <min_size> <max_size>\n");
    return 2;
  }
  try {
    const auto cloud = read_cloud(argv[1]);
    rgc::EuclideanClusterExtractionHip ec(0);
    ec.setInputCloud(cloud);
    ec.setClusterTolerance(std::atof(argv[2]));
    ec.setMinClusterSize(std::atoi(argv[3]));
    ec.setMaxClusterSize(std::atoi(argv[4]));
    std::vector<std::vector<int>> clusters;
    ec.extract(clusters);
    print_row("M", std::vector<int>(1, (int)clusters.size()));
    for (const std::vector<int>& c : clusters) print_row("C", c);
    print_row("L", ec.labels());
    const rgc_cluster_info info = ec.info();
    const std::vector<std::vector<int>> first = clusters;
    rgc::EuclideanClusterExtractionHip again(ec.context());   // in the same context: the same clusters
    again.setInputCloud(cloud);
    again.setClusterTolerance(ec.getClusterTolerance());
    again.setMinClusterSize(ec.getMinClusterSize());
    again.setMaxClusterSize(ec.getMaxClusterSize());
    std::vector<std::vector<int>> twice;
    again.extract(twice);
    int threw = 0;
    try { ec.setClusterTolerance(-1.0); } catch (const std::runtime_error&) { threw++; }
    try { ec.setMinClusterSize(0); } catch (const std::runtime_error&) { threw++; }
    try { ec.setMinClusterSize(5); ec.setMaxClusterSize(4); ec.extract(clusters); } catch (const std::runtime_error&) { threw++; }   // max < min: the call is refused
    std::fprintf(stderr, "%d points, %d components, %d clusters of %d points, largest %d, cell %g, %lld cells\n", info.n, info.n_components, info.n_clusters, info.n_clustered,
                 info.largest, info.cell, info.cells);
    return threw == 3 && twice == first && twice.size() == (size_t)info.n_clusters && info.n == (int)cloud->points.size() ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
}
