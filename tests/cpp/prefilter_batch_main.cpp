// A plain C++ caller of hgs_prefilter_batch (include/hgs_registration.h), no adapter: several sweeps through the prefilter in one device batch.
//   prefilter_batch_main <downsample_method> <downsample_resolution> <outlier_removal_method> <radius_radius> <radius_min_neighbors> <cloud.bin>:<meta.bin> ...
// Every sweep is a file of pcl::PointXYZI records (32 bytes) and a file of 6 doubles {has gyro sample, w[3], scan period, has matrix} followed by the 16
// floats of sensor_to_base (column-major).  Prints one line per sweep: "<sweep> <points> <FNV-1a of the x, y, z, intensity bits> identical <0|1>" — the
// last field says whether hgs_prefilter_framed of that sweep alone, on a second engine, gave the same records.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/hgs_registration.h"

static std::vector<char> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) {
    std::fprintf(stderr, "cannot read %s\n", path.c_str());
    std::exit(2);
  }
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct Sweep {
  std::vector<char> pts;
  double extras[6];
  float matrix[16];
};

// the records of a resident cloud as packed {x, y, z, intensity} bit patterns
static std::vector<uint32_t> records(hgs_cloud* c) {
  const size_t n = hgs_cloud_size(c);
  std::vector<float> xyzi(8 * (n + 1));
  if (hgs_cloud_download(c, xyzi.data(), 32) != HGS_OK) std::exit(1);
  std::vector<uint32_t> out(4 * n);
  for (size_t i = 0; i < n; i++) {
    const float f[4] = {xyzi[8 * i], xyzi[8 * i + 1], xyzi[8 * i + 2], xyzi[8 * i + 4]};
    std::memcpy(&out[4 * i], f, 16);
  }
  return out;
}

int main(int argc, char** argv) {
  if (argc < 7) {
    std::fprintf(stderr, "usage: prefilter_batch_main <downsample> <resolution> <outlier> <radius> <min_neighbors> <cloud.bin>:<meta.bin> ...\n");
    return 2;
  }
  hgs_prefilter_params p;
  hgs_prefilter_params_default(&p);
  p.downsample_method = std::atoi(argv[1]), p.downsample_resolution = std::atof(argv[2]);
  p.outlier_removal_method = std::atoi(argv[3]), p.radius_radius = std::atof(argv[4]), p.radius_min_neighbors = std::atoi(argv[5]);
  std::vector<Sweep> data(argc - 6);
  for (int i = 6; i < argc; i++) {
    const std::string tok = argv[i];
    const size_t colon = tok.rfind(':');
    if (colon == std::string::npos) {
      std::fprintf(stderr, "bad token %s\n", tok.c_str());
      return 2;
    }
    Sweep& s = data[i - 6];
    s.pts = slurp(tok.substr(0, colon));
    const std::vector<char> meta = slurp(tok.substr(colon + 1));
    if (meta.size() != sizeof(s.extras) + sizeof(s.matrix)) {
      std::fprintf(stderr, "%s: expected 6 doubles and 16 floats\n", tok.c_str());
      return 2;
    }
    std::memcpy(s.extras, meta.data(), sizeof(s.extras));
    std::memcpy(s.matrix, meta.data() + sizeof(s.extras), sizeof(s.matrix));
  }
  hgs_params rp;
  hgs_params_default(HGS_FAST_GICP, &rp);
  hgs_handle *h = nullptr, *h1 = nullptr;
  if (hgs_create(&rp, &h) != HGS_OK || hgs_create(&rp, &h1) != HGS_OK) {
    std::fprintf(stderr, "hgs_create failed: %s\n", hgs_last_error(nullptr));
    return 1;
  }
  std::vector<hgs_prefilter_sweep> sweeps(data.size());
  for (size_t i = 0; i < data.size(); i++) {
    const Sweep& s = data[i];
    sweeps[i].pts = s.pts.data(), sweeps[i].n = s.pts.size() / 32, sweeps[i].stride_bytes = 32;
    sweeps[i].imu_angular_velocity = s.extras[0] != 0 ? &s.extras[1] : nullptr;
    sweeps[i].scan_period = s.extras[4];
    sweeps[i].sensor_to_base = s.extras[5] != 0 ? s.matrix : nullptr;
  }
  std::vector<hgs_cloud*> out(sweeps.size(), nullptr);
  if (hgs_prefilter_batch(h, sweeps.data(), sweeps.size(), &p, out.data()) != HGS_OK) {
    std::fprintf(stderr, "hgs_prefilter_batch failed: %s\n", hgs_last_error(h));
    return 1;
  }
  for (size_t i = 0; i < sweeps.size(); i++) {
    const hgs_prefilter_sweep& s = sweeps[i];
    hgs_cloud* one = nullptr;
    if (hgs_prefilter_framed(h1, s.pts, s.n, s.stride_bytes, &p, s.imu_angular_velocity, s.scan_period, s.sensor_to_base, &one) != HGS_OK) {
      std::fprintf(stderr, "hgs_prefilter_framed failed: %s\n", hgs_last_error(h1));
      return 1;
    }
    const std::vector<uint32_t> a = records(out[i]), b = records(one);
    uint64_t sum = 1469598103934665603ull;
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(a.data());
    for (size_t k = 0; k < a.size() * 4; k++) sum = (sum ^ bytes[k]) * 1099511628211ull;
    std::printf("%zu %zu %016llx identical %d\n", i, a.size() / 4, (unsigned long long)sum, a == b ? 1 : 0);
    hgs_cloud_destroy(one);
    hgs_cloud_destroy(out[i]);
  }
  hgs_destroy(h);
  hgs_destroy(h1);
  return 0;
}
