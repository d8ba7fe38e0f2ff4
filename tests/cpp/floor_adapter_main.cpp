// TEST ONLY — adapters/floor_detection_hip.hpp driven like FloorDetectionNodelet::cloud_callback drives detect() (apps/floor_detection_nodelet.cpp:72-81).
// Usage: floor_adapter_main <use_normal_filtering 0|1> <seed> <cloud.bin> [raw.bin]   (raw PointXYZI records)
// With raw.bin the sweep first goes through ResidentCloudsHIP::prefilter (the nodelet's defaults) and the floor is detected on its output, which the
// detector finds resident.  Prints: detected / reason / counts / iterations, the coefficients as float bit patterns, the resident hits.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <pcl/point_types.h>
#include "../../adapters/floor_detection_hip.hpp"

using PointT = pcl::PointXYZI;

static pcl::PointCloud<PointT> load(const char* path) {
  pcl::PointCloud<PointT> c;
  FILE* f = std::fopen(path, "rb");
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  PointT p;
  while (std::fread(&p, sizeof(PointT), 1, f) == 1) c.points.push_back(p);
  std::fclose(f);
  return c;
}

static void print(const hgs_hip::FloorDetector<PointT>& fd, bool found, const Eigen::Vector4f& co, const pcl::PointCloud<PointT>& filtered, const pcl::PointCloud<PointT>& inliers) {
  const hgs_floor_result& r = fd.lastResult();
  std::printf("ran %d detected %d reason %d clipped %u filtered %u inliers %u iterations %d\n", (int)fd.device_ran(), (int)found, r.reason, r.n_clipped, r.n_filtered,
              r.n_inliers, r.ransac_iterations);
  std::printf("coeffs");
  for (int i = 0; i < 4; i++) {
    unsigned bits;
    const float v = found ? co[i] : 0.f;
    std::memcpy(&bits, &v, 4);
    std::printf(" %08x", bits);
  }
  std::printf("\nclouds %zu %zu\n", filtered.points.size(), inliers.points.size());
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s use_normal_filtering seed cloud.bin [raw.bin]\n", argv[0]);
    return 2;
  }
  try {
    hgs_hip::FloorDetector<PointT> fd;
    fd.use_normal_filtering = std::atoi(argv[1]) != 0;
    fd.seed = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    pcl::PointCloud<PointT> cloud = load(argv[3]), filtered, inliers;
    Eigen::Vector4f co;
    bool found = fd.detect(cloud, co, &filtered, &inliers);
    print(fd, found, co, filtered, inliers);
    auto& rc = hgs_hip::ResidentCloudsHIP<PointT>::instance();
    std::printf("resident_hits %zu\n", rc.resident_hits());
    if (argc > 4) {
      pcl::PointCloud<PointT> raw = load(argv[4]), pre;
      hgs_prefilter_params pp;
      hgs_prefilter_params_default(&pp);
      if (!rc.prefilter(raw, pp, nullptr, 0.1, pre)) throw std::runtime_error("prefilter: " + rc.last_error());
      found = fd.detect(pre, co, &filtered, &inliers);
      std::printf("prefiltered %zu\n", pre.points.size());
      print(fd, found, co, filtered, inliers);
      std::printf("resident_hits %zu\n", rc.resident_hits());
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
