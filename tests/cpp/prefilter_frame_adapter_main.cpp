// TEST ONLY — ResidentCloudsHIP::prefilter with a base_link transform, driven as PrefilteringNodelet::cloud_callback would drive it
// (apps/prefiltering_nodelet.cpp:114-133), in two ways on the same sweep:
//   1. the matrix goes to the device (the overload with `sensor_to_base`),
//   2. the mock pcl::transformPointCloud (PCL >= 1.10's order) runs on the host first and no matrix is passed.
// Usage: prefilter_frame_adapter_main <raw.bin: PointXYZI records> <matrix.bin: 16 floats, column-major> <downsample_method> <outlier_removal_method>
// Prints: the two sizes, whether the two clouds are identical in every bit of x, y, z and intensity, and a checksum of the first one's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <pcl/point_types.h>
#include <pcl/common/transforms.h>
#include "../../adapters/resident_clouds_hip.hpp"

using PointT = pcl::PointXYZI;

static uint64_t checksum(const pcl::PointCloud<PointT>& c) {  // FNV-1a over the bits of x, y, z, intensity of every point, in order
  uint64_t h = 1469598103934665603ull;
  for (const PointT& p : c.points) {
    const float v[4] = {p.x, p.y, p.z, p.intensity};
    unsigned char b[16];
    std::memcpy(b, v, 16);
    for (unsigned char byte : b) h = (h ^ byte) * 1099511628211ull;
  }
  return h;
}

int main(int argc, char** argv) {
  if (argc != 5) {
    std::fprintf(stderr, "usage: %s raw.bin matrix.bin downsample_method outlier_removal_method\n", argv[0]);
    return 2;
  }
  try {
    pcl::PointCloud<PointT> raw, moved, a, b;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + argv[1]);
    PointT p;
    while (std::fread(&p, sizeof(PointT), 1, f) == 1) raw.points.push_back(p);
    std::fclose(f);
    Eigen::Matrix4f m;
    f = std::fopen(argv[2], "rb");
    if (!f || std::fread(m.data(), sizeof(float), 16, f) != 16) throw std::runtime_error(std::string("cannot read ") + argv[2]);
    std::fclose(f);
    hgs_prefilter_params pp;
    hgs_prefilter_params_default(&pp);
    pp.downsample_method = std::atoi(argv[3]);
    pp.outlier_removal_method = std::atoi(argv[4]);
    auto& rc = hgs_hip::ResidentCloudsHIP<PointT>::instance();
    if (!rc.prefilter(raw, pp, nullptr, 0.1, m.data(), a)) throw std::runtime_error("prefilter with the matrix: " + rc.last_error());
    pcl::transformPointCloud(raw, moved, m);
    if (!rc.prefilter(moved, pp, nullptr, 0.1, b)) throw std::runtime_error("prefilter of the transformed sweep: " + rc.last_error());
    bool same = a.points.size() == b.points.size();
    for (size_t i = 0; same && i < a.points.size(); i++) {
      const float u[4] = {a.points[i].x, a.points[i].y, a.points[i].z, a.points[i].intensity}, v[4] = {b.points[i].x, b.points[i].y, b.points[i].z, b.points[i].intensity};
      same = std::memcmp(u, v, 16) == 0;
    }
    std::printf("raw %zu framed %zu host_transformed %zu identical %d checksum %016llx device_calls %zu\n", raw.points.size(), a.points.size(), b.points.size(), (int)same,
                (unsigned long long)checksum(a), rc.device_calls());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
