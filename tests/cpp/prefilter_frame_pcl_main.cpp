// TEST ONLY — the mock pcl::transformPointCloud (tests/mock_pcl/pcl/common/transforms.h, PCL >= 1.10's order) on a file of PointXYZI records: what
// tests/prefilter_frame_reference.py is held to, bit for bit.  Compiled with -ffp-contract=off.
// Usage: prefilter_frame_pcl_main <cloud.bin> <matrix.bin: 16 floats, column-major> <out.bin>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <pcl/point_types.h>
#include <pcl/common/transforms.h>

using PointT = pcl::PointXYZI;

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s cloud.bin matrix.bin out.bin\n", argv[0]);
    return 2;
  }
  try {
    pcl::PointCloud<PointT> in, out;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + argv[1]);
    PointT p;
    while (std::fread(&p, sizeof(PointT), 1, f) == 1) in.points.push_back(p);
    std::fclose(f);
    Eigen::Matrix4f m;
    f = std::fopen(argv[2], "rb");
    if (!f || std::fread(m.data(), sizeof(float), 16, f) != 16) throw std::runtime_error(std::string("cannot read ") + argv[2]);
    std::fclose(f);
    pcl::transformPointCloud(in, out, m);
    f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(out.points.data(), sizeof(PointT), out.points.size(), f) != out.points.size()) throw std::runtime_error(std::string("cannot write ") + argv[3]);
    std::fclose(f);
    std::printf("points %zu\n", out.points.size());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
