// rgc::FPFHEstimationHip (rgc-slam_amd/cpp/features_hip.hpp) used the way a caller of pcl::FPFHEstimation would: pcl-style clouds, setInputCloud,
// setSearchSurface, setInputNormals, setRadiusSearch, compute.  Compiled -Wall -Wextra -Werror by tests/test_fpfh_api.py (no GPU needed for that);
// tests/test_gpu_cpp_fpfh.py runs it on a GPU with files of float32 rows and compares the lines it prints with the numpy reference and with the C-ABI
// called directly.
// usage: test_fpfh <cloud.f32> <surface.f32 | -> <normals.f32> <radius>
// Line format: <tag> <count> then the values; tags: F the descriptors (33 per point, hex floats), H the SPFH counts, C the SPFH row sizes, M the queries'
// row sizes, A / B the descriptors and the row sizes from rgc_fpfh_estimate itself, V the number of valid rows (the adaptor's, the C-ABI's) and n_spfh.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../rgc-slam_amd/cpp/features_hip.hpp"

struct Point { float x, y, z, intensity; };
struct Cloud { std::vector<Point> points; };
struct Normal { float normal_x, normal_y, normal_z, curvature; };
struct Normals { std::vector<Normal> points; };

static std::vector<float> read_file(const char* path) {
  std::vector<float> v;
  std::FILE* f = std::fopen(path, "rb");
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  float x;
  while (std::fread(&x, sizeof(float), 1, f) == 1) v.push_back(x);
  std::fclose(f);
  return v;
}
static std::shared_ptr<Cloud> cloud_of(const std::vector<float>& xyz) {
  auto cloud = std::make_shared<Cloud>();
  for (size_t i = 0; i + 2 < xyz.size(); i += 3) cloud->points.push_back(Point{xyz[i], xyz[i + 1], xyz[i + 2], (float)(i / 3)});
  return cloud;
}
static std::shared_ptr<Normals> normals_of(const std::vector<float>& xyz) {
  auto normals = std::make_shared<Normals>();
  for (size_t i = 0; i + 2 < xyz.size(); i += 3) normals->points.push_back(Normal{xyz[i], xyz[i + 1], xyz[i + 2], 0.f});
  return normals;
}
template <typename T> static void print_ints(const char* tag, const std::vector<T>& v) {
  std::printf("%s %zu", tag, v.size());
  for (T x : v) std::printf(" %lld", (long long)x);
  std::printf("\n");
}
static void print_reals(const char* tag, const std::vector<float>& v) {
  std::printf("%s %zu", tag, v.size());
  for (float x : v) std::printf(" %a", (double)x);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: test_fpfh <cloud.f32> <surface.f32 | -> <normals.f32> <radius>\n");
    return 2;
  }
  try {
    auto cloud = cloud_of(read_file(argv[1]));
    const bool with_surface = argv[2][0] != '-';
    auto surface = with_surface ? cloud_of(read_file(argv[2])) : std::make_shared<Cloud>();
    auto normals = normals_of(read_file(argv[3]));
    const double radius = std::atof(argv[4]);
    rgc::FPFHEstimationHip fe(0);
    fe.setInputCloud(cloud);
    if (with_surface) fe.setSearchSurface(surface);
    fe.setInputNormals(normals);
    fe.setRadiusSearch(radius);
    std::vector<float> fpfh;
    std::vector<unsigned> spfh;
    std::vector<int> spfh_count, count;
    const int valid = fe.compute(fpfh, &spfh, &spfh_count, &count);
    print_reals("F", fpfh);
    print_ints("H", spfh);
    print_ints("C", spfh_count);
    print_ints("M", count);
    const rgc_fpfh_info info = fe.info();
    // the C-ABI itself, in the same context
    rgc_fpfh_params p;
    rgc_default_fpfh_params(&p);
    p.radius = fe.getRadiusSearch();
    const size_t n = cloud->points.size();
    std::vector<float> direct(n * RGC_FPFH_BINS, 0.f);
    std::vector<int> direct_count(n, 0);
    int m = 0;
    const int rc = rgc_fpfh_estimate(fe.context(), &cloud->points[0].x, (int)n, (int)sizeof(Point), with_surface ? &surface->points[0].x : nullptr, (int)surface->points.size(),
                                     (int)sizeof(Point), &normals->points[0].normal_x, (int)sizeof(Normal), 0, &p, direct.data(), nullptr, nullptr, direct_count.data(), &m);
    print_reals("A", direct);
    print_ints("B", direct_count);
    print_ints("V", std::vector<int>{valid, m, info.n_spfh});
    // compute(fpfh) alone gives the same rows, and so do the normals handed over as a strided float array
    std::vector<float> again, strided;
    const int valid2 = fe.compute(again);
    fe.setInputNormals(&normals->points[0].normal_x, (int)normals->points.size(), (int)sizeof(Normal));
    const int valid3 = fe.compute(strided);
    int threw = 0;
    try { fe.setRadiusSearch(0.0); } catch (const std::runtime_error&) { threw++; }
    try { fe.setRadiusSearch(-1.0); } catch (const std::runtime_error&) { threw++; }
    try { fe.setRadiusSearch(std::nan("")); } catch (const std::runtime_error&) { threw++; }
    try { fe.setInputNormals(&normals->points[0].normal_x, 1, 16); fe.compute(again); } catch (const std::runtime_error&) { threw++; }
    std::fprintf(stderr, "%d queries against %d surface points, %d valid, %d SPFHs, cell %g, %lld cells, %lld pairs, %lld candidates\n", info.n, info.n_surface, info.n_valid,
                 info.n_spfh, info.cell, info.cells, info.pairs, info.candidates);
    const size_t bytes = n * RGC_FPFH_BINS * sizeof(float);
    const bool same = rc == RGC_OK && valid == m && valid2 == m && valid3 == m && info.n == (int)n && info.n_valid == m && count == direct_count &&
                      std::memcmp(direct.data(), fpfh.data(), bytes) == 0 && std::memcmp(strided.data(), fpfh.data(), bytes) == 0;
    return threw == 4 && same && fe.getRadiusSearch() == radius ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
}
