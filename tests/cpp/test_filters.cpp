// rgc::StatisticalOutlierRemovalHip / rgc::RadiusOutlierRemovalHip (rgc-slam_amd/cpp/filters_hip.hpp) used the way a caller of the PCL filters would:
// a pcl-style cloud, setInputCloud, the setters, filter(cloud) and filter(indices), setNegative, getRemovedIndices.  Compiled -Wall -Wextra -Werror by
// tests/test_outlier_api.py (no GPU needed for that); tests/test_gpu_cpp_filters.py runs it on a GPU with a file of float32 x, y, z rows and compares the
// lines it prints with the numpy reference for equality.  usage: test_filters <cloud.f32> <mean_k> <std_mul> <radius> <min_neighbors>
// Line format: <tag> <count> then the values; tags: S / s kept and removed indices of SOR, N SOR's kept indices with setNegative(true), D the mean distances'
// bit patterns, R / r kept and removed indices of ROR, C the counts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../rgc-slam_amd/cpp/filters_hip.hpp"

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
template <typename T> static void print_row(const char* tag, const std::vector<T>& v) {
  std::printf("%s %zu", tag, v.size());
  for (const T& x : v) {
    unsigned u;
    std::memcpy(&u, &x, sizeof(u));
    std::printf(" %u", u);
  }
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: test_filters <cloud.f32> <mean_k> <std_mul> <radius> <min_neighbors>\n");
    return 2;
  }
  try {
    const auto cloud = read_cloud(argv[1]);
    rgc::StatisticalOutlierRemovalHip sor(0);
    sor.setInputCloud(cloud);
    sor.setMeanK(std::atoi(argv[2]));
    sor.setStddevMulThresh(std::atof(argv[3]));
    Cloud out;
    sor.filter(out);
    std::vector<int> idx;
    sor.filter(idx);
    if (idx.size() != out.points.size()) return 1;
    for (size_t j = 0; j < idx.size(); j++)      // the output's points are the input's, intensity (here: the index) included
      if (std::memcmp(&out.points[j], &cloud->points[(size_t)idx[j]], sizeof(Point)) != 0 || out.points[j].intensity != (float)idx[j]) return 1;
    print_row("S", idx);
    print_row("s", sor.getRemovedIndices());
    print_row("D", sor.meanDistances());
    const rgc_outlier_info si = sor.info();
    sor.setNegative(true);
    sor.filter(idx);
    print_row("N", idx);
    rgc::RadiusOutlierRemovalHip ror(sor.context());   // in the same context
    ror.setInputCloud(cloud);
    ror.setRadiusSearch(std::atof(argv[4]));
    ror.setMinNeighborsInRadius(std::atoi(argv[5]));
    ror.filter(out);
    ror.filter(idx);
    if (idx.size() != out.points.size()) return 1;
    print_row("R", idx);
    print_row("r", ror.getRemovedIndices());
    print_row("C", ror.counts());
    int threw = 0;
    try { sor.setMeanK(RGC_OUTLIER_MAX_MEAN_K + 1); } catch (const std::runtime_error&) { threw++; }
    try { ror.setRadiusSearch(-1.0); } catch (const std::runtime_error&) { threw++; }
    try { sor.setMeanK((int)cloud->points.size()); sor.filter(idx); } catch (const std::runtime_error&) { threw++; }   // n <= mean_k: the call is refused
    std::fprintf(stderr, "%d points, SOR kept %d (mean %.9g stddev %.9g threshold %.17g), cell %g, %lld cells\n", si.n, si.n_out, si.mean, si.stddev, si.threshold, si.cell, si.cells);
    return threw == 3 && si.n == (int)cloud->points.size() ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
}
