// A plain C++ caller of hgs_detect_floor_batch (include/hgs_registration.h), no adapter: the floor plane of several resident clouds in one device batch.
//   floor_batch_main <use_normal_filtering> <floor_pts_thresh> <cloud.bin> ...
// Every cloud is a file of pcl::PointXYZI records (32 bytes).  Prints one line per cloud:
//   "<cloud> <detected> <reason> <n_clipped> <n_filtered> <n_inliers> <ransac_iterations> <the four coefficients' bits> <filtered points> <FNV-1a of their
//    x, y, z, intensity bits> <inlier points or -1> <FNV-1a of theirs> identical <0|1>"
// — the last field says whether hgs_detect_floor of that cloud alone, on a second engine, gave the same record and the same two clouds — and a last line
//   "stats <clouds> <ransac_clouds> <ransac_rounds> <readbacks>" from hgs_debug_floor_batch_stats.
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

// the records of a resident cloud as packed {x, y, z, intensity} bit patterns (NULL: none)
static std::vector<uint32_t> records(hgs_cloud* c) {
  if (!c) return {};
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

static unsigned long long fnv1a(const std::vector<uint32_t>& a) {
  uint64_t sum = 1469598103934665603ull;
  const unsigned char* bytes = reinterpret_cast<const unsigned char*>(a.data());
  for (size_t k = 0; k < a.size() * 4; k++) sum = (sum ^ bytes[k]) * 1099511628211ull;
  return (unsigned long long)sum;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: floor_batch_main <use_normal_filtering> <floor_pts_thresh> <cloud.bin> ...\n");
    return 2;
  }
  hgs_floor_params p;
  hgs_floor_params_default(&p);
  p.use_normal_filtering = std::atoi(argv[1]), p.floor_pts_thresh = std::atoi(argv[2]);
  hgs_params rp;
  hgs_params_default(HGS_FAST_GICP, &rp);
  hgs_handle *h = nullptr, *h1 = nullptr;
  if (hgs_create(&rp, &h) != HGS_OK || hgs_create(&rp, &h1) != HGS_OK) {
    std::fprintf(stderr, "hgs_create failed: %s\n", hgs_last_error(nullptr));
    return 1;
  }
  const size_t n = (size_t)argc - 3;
  std::vector<std::vector<char>> data(n);
  std::vector<hgs_cloud*> clouds(n, nullptr), clouds1(n, nullptr);
  for (size_t i = 0; i < n; i++) {
    data[i] = slurp(argv[3 + i]);
    if (hgs_cloud_create(h, data[i].data(), data[i].size() / 32, 32, &clouds[i]) != HGS_OK ||
        hgs_cloud_create(h1, data[i].data(), data[i].size() / 32, 32, &clouds1[i]) != HGS_OK) {
      std::fprintf(stderr, "hgs_cloud_create failed: %s\n", hgs_last_error(h));
      return 1;
    }
  }
  std::vector<hgs_floor_result> out(n);
  std::vector<hgs_cloud*> filtered(n, nullptr), inliers(n, nullptr);
  if (hgs_detect_floor_batch(h, clouds.data(), n, &p, out.data(), filtered.data(), inliers.data()) != HGS_OK) {
    std::fprintf(stderr, "hgs_detect_floor_batch failed: %s\n", hgs_last_error(h));
    return 1;
  }
  for (size_t i = 0; i < n; i++) {
    hgs_floor_result one;
    hgs_cloud *f1 = nullptr, *i1 = nullptr;
    if (hgs_detect_floor(h1, clouds1[i], &p, &one, &f1, &i1) != HGS_OK) {
      std::fprintf(stderr, "hgs_detect_floor failed: %s\n", hgs_last_error(h1));
      return 1;
    }
    const std::vector<uint32_t> fa = records(filtered[i]), fb = records(f1), ia = records(inliers[i]), ib = records(i1);
    const bool same = std::memcmp(&one, &out[i], sizeof(one)) == 0 && fa == fb && ia == ib && (inliers[i] == nullptr) == (i1 == nullptr) && filtered[i] && f1;
    uint32_t co[4];
    std::memcpy(co, out[i].coeffs, 16);
    std::printf("%zu %d %d %u %u %u %d %08x %08x %08x %08x %zu %016llx %ld %016llx identical %d\n", i, out[i].detected, out[i].reason, out[i].n_clipped, out[i].n_filtered,
                out[i].n_inliers, out[i].ransac_iterations, co[0], co[1], co[2], co[3], fa.size() / 4, fnv1a(fa), inliers[i] ? (long)(ia.size() / 4) : -1L, fnv1a(ia),
                same ? 1 : 0);
    hgs_cloud_destroy(f1);
    hgs_cloud_destroy(i1);
    hgs_cloud_destroy(filtered[i]);
    hgs_cloud_destroy(inliers[i]);
    hgs_cloud_destroy(clouds[i]);
    hgs_cloud_destroy(clouds1[i]);
  }
  int32_t s[4] = {0, 0, 0, 0};
  hgs_debug_floor_batch_stats(h, &s[0], &s[1], &s[2], &s[3]);
  std::printf("stats %d %d %d %d\n", s[0], s[1], s[2], s[3]);
  hgs_destroy(h);
  hgs_destroy(h1);
  return 0;
}
