// rgc::SACSegmentationHip (rgc-slam_amd/cpp/segmentation_hip.hpp) used the way a caller of pcl::SACSegmentation + pcl::ExtractIndices would: a pcl-style
// cloud, setInputCloud, the setters, segment(inliers, coefficients), filter(rest).  Compiled -Wall -Wextra -Werror by tests/test_plane_api.py (no GPU
// needed for that); tests/test_gpu_cpp_plane.py runs it on a GPU with a file of float32 x, y, z rows and a file of int32 sample triples and compares the
// lines it prints with the numpy reference and with the C-ABI called directly.
// usage: test_plane <cloud.f32> <samples.i32 | -> <threshold> <max_iterations> <optimize> <seed> <model: 0 | 11> <ax> <ay> <az> <eps_angle>
// Line format: <tag> <count> then the values; tags: I the inliers, C the coefficients (hex floats), A / D the same two from rgc_plane_segment itself,
// N the complement's indices recovered from filter()'s records (their c holds the input index).
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../rgc-slam_amd/cpp/segmentation_hip.hpp"

struct Point { float x, y, z, intensity; };
struct Cloud { std::vector<Point> points; };

template <typename T> static std::vector<T> read_file(const char* path) {
  std::vector<T> v;
  std::FILE* f = std::fopen(path, "rb");
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  T x;
  while (std::fread(&x, sizeof(T), 1, f) == 1) v.push_back(x);
  std::fclose(f);
  return v;
}
static void print_ints(const char* tag, const std::vector<int>& v) {
  std::printf("%s %zu", tag, v.size());
  for (int x : v) std::printf(" %d", x);
  std::printf("\n");
}
template <typename T> static void print_reals(const char* tag, const std::vector<T>& v) {
  std::printf("%s %zu", tag, v.size());
  for (T x : v) std::printf(" %a", (double)x);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 12) {
    std::fprintf(stderr, "usage: test_plane <cloud.f32> <samples.i32 | -> <threshold> <max_iterations> <optimize> <seed> <model> <ax> <ay> <az> <eps_angle>\n");
    return 2;
  }
  try {
    const std::vector<float> xyz = read_file<float>(argv[1]);
    auto cloud = std::make_shared<Cloud>();
    for (size_t i = 0; i + 2 < xyz.size(); i += 3) cloud->points.push_back(Point{xyz[i], xyz[i + 1], xyz[i + 2], (float)(i / 3)});
    const std::vector<int> samples = argv[2][0] == '-' ? std::vector<int>() : read_file<int>(argv[2]);
    rgc::SACSegmentationHip seg(0);
    seg.setInputCloud(cloud);
    seg.setModelType(std::atoi(argv[7]));
    seg.setMethodType(rgc::SAC_RANSAC);
    seg.setDistanceThreshold(std::atof(argv[3]));
    seg.setMaxIterations(std::atoi(argv[4]));
    seg.setOptimizeCoefficients(std::atoi(argv[5]) != 0);
    seg.setSeed(std::strtoull(argv[6], nullptr, 10));
    if (seg.getModelType() == rgc::SACMODEL_PERPENDICULAR_PLANE) {
      seg.setAxis(std::atof(argv[8]), std::atof(argv[9]), std::atof(argv[10]));
      seg.setEpsAngle(std::atof(argv[11]));
    }
    seg.setSamples(samples);
    std::vector<int> inliers;
    std::vector<float> coefficients;
    seg.segment(inliers, coefficients);
    print_ints("I", inliers);
    print_reals("C", coefficients);
    const rgc_plane_info info = seg.info();
    // the C-ABI itself, in the same context
    rgc_plane_params p;
    rgc_default_plane_params(&p);
    p.distance_threshold = seg.getDistanceThreshold(); p.max_iterations = seg.getMaxIterations(); p.optimize = seg.getOptimizeCoefficients() ? 1 : 0;
    p.seed = std::strtoull(argv[6], nullptr, 10);
    if (seg.getModelType() == rgc::SACMODEL_PERPENDICULAR_PLANE) {
      p.model_type = RGC_PLANE_PERPENDICULAR; p.axis[0] = std::atof(argv[8]); p.axis[1] = std::atof(argv[9]); p.axis[2] = std::atof(argv[10]); p.eps_angle = seg.getEpsAngle();
    }
    std::vector<int> direct(cloud->points.size(), 0);
    std::vector<double> coeff(4, 0.0);
    int m = 0;
    const int rc = rgc_plane_segment(seg.context(), &cloud->points[0].x, (int)cloud->points.size(), (int)sizeof(Point), 0, &p, samples.empty() ? nullptr : samples.data(),
                                     (int)(samples.size() / 3), 0, coeff.data(), nullptr, direct.data(), nullptr, &m);
    direct.resize((size_t)m);
    print_ints("A", direct);
    print_reals("D", coeff);
    // the ExtractIndices step: everything else, in input order (the records' fourth float is the input index here)
    seg.setNegative(true);
    std::vector<float> rest;
    seg.filter(rest);
    std::vector<int> rest_index;
    for (size_t i = 0; i + 3 < rest.size(); i += 4) rest_index.push_back((int)rest[i + 3]);
    print_ints("N", rest_index);
    int threw = 0;
    try { seg.setDistanceThreshold(0.0); } catch (const std::runtime_error&) { threw++; }
    try { seg.setMethodType(1); } catch (const std::runtime_error&) { threw++; }
    try { seg.setModelType(5); } catch (const std::runtime_error&) { threw++; }
    try { seg.setBatch(-1); } catch (const std::runtime_error&) { threw++; }
    std::fprintf(stderr, "%d points, %d inliers, %d iterations, %lld positions (%lld skipped), best %lld with %d, k %g, batch %d, %d launches, refined %d\n", info.n, info.n_inliers,
                 info.iterations, info.positions, info.skipped, info.best_position, info.best_count, info.k, info.batch, info.launches, info.refined);
    bool same = rc == RGC_OK && direct == inliers && info.n == (int)cloud->points.size() && info.n_inliers == (int)inliers.size();
    for (size_t a = 0; a < coefficients.size(); a++) same = same && (double)coefficients[a] == coeff[a];
    return threw == 4 && same && rest_index.size() + inliers.size() == cloud->points.size() ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
}
