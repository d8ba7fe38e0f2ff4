// A plain C++ caller of hgs_align_pairs (include/hgs_registration.h), no adapter: n independent registrations (target i, source i, guess i) in one batch.
//   align_pairs_main <method> <neighbor_search> <resolution> <max_range> <guesses.bin> C:<cloud.bin> ... P:<target>:<source> ...
// Every C token is a cloud of pcl::PointXYZI records (32 bytes), numbered in token order; every P token is a pair of cloud numbers; guesses.bin holds 16
// floats (column-major) per pair in token order.  resolution <= 0 keeps the method's default.  Prints one line per record, "<tag> <pair> <the hgs_result
// as hex>": tag F for the call with getFitnessScore(max_range) behind every registration, N for the call without (max_range NULL).
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

static void print(const char* tag, const std::vector<hgs_result>& records) {
  for (size_t i = 0; i < records.size(); i++) {
    std::printf("%s %zu ", tag, i);
    const unsigned char* b = reinterpret_cast<const unsigned char*>(&records[i]);
    for (size_t k = 0; k < sizeof(hgs_result); k++) std::printf("%02x", b[k]);
    std::printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc < 8) {
    std::fprintf(stderr, "usage: align_pairs_main <method> <neighbor_search> <resolution> <max_range> <guesses.bin> C:<cloud.bin> ... P:<target>:<source> ...\n");
    return 2;
  }
  hgs_params p;
  hgs_params_default(std::atoi(argv[1]), &p);
  p.neighbor_search = std::atoi(argv[2]);
  if (std::atof(argv[3]) > 0) p.resolution = std::atof(argv[3]);
  const double max_range = std::atof(argv[4]);
  const std::vector<char> guesses = slurp(argv[5]);
  hgs_handle* h = nullptr;
  if (hgs_create(&p, &h) != HGS_OK) {
    std::fprintf(stderr, "hgs_create failed: %s\n", hgs_last_error(nullptr));
    return 1;
  }
  std::vector<hgs_cloud*> clouds, targets, sources;
  for (int i = 6; i < argc; i++) {
    const std::string tok = argv[i];
    if (tok.size() > 2 && tok[0] == 'C' && tok[1] == ':') {
      const std::vector<char> pts = slurp(tok.substr(2));
      hgs_cloud* c = nullptr;
      if (hgs_cloud_create(h, pts.data(), pts.size() / 32, 32, &c) != HGS_OK) {
        std::fprintf(stderr, "hgs_cloud_create failed: %s\n", hgs_last_error(h));
        return 1;
      }
      clouds.push_back(c);
      continue;
    }
    const size_t c2 = tok.find(':', 2);
    if (tok.size() < 5 || tok[0] != 'P' || tok[1] != ':' || c2 == std::string::npos) {
      std::fprintf(stderr, "bad token %s\n", tok.c_str());
      return 2;
    }
    const size_t t = (size_t)std::atol(tok.substr(2, c2 - 2).c_str()), s = (size_t)std::atol(tok.substr(c2 + 1).c_str());
    if (t >= clouds.size() || s >= clouds.size()) {
      std::fprintf(stderr, "pair %s names a cloud that has not been given\n", tok.c_str());
      return 2;
    }
    targets.push_back(clouds[t]), sources.push_back(clouds[s]);
  }
  const size_t n = targets.size();
  if (guesses.size() < n * 64) {
    std::fprintf(stderr, "guesses.bin is too short\n");
    return 2;
  }
  const float* g = reinterpret_cast<const float*>(guesses.data());
  std::vector<hgs_result> with_fitness(n), without(n);
  if (hgs_align_pairs(h, targets.data(), sources.data(), g, &max_range, n, with_fitness.data()) != HGS_OK ||
      hgs_align_pairs(h, targets.data(), sources.data(), g, nullptr, n, without.data()) != HGS_OK) {
    std::fprintf(stderr, "hgs_align_pairs failed: %s\n", hgs_last_error(h));
    return 1;
  }
  print("F", with_fitness);
  print("N", without);
  for (hgs_cloud* c : clouds) hgs_cloud_destroy(c);
  hgs_destroy(h);
  return 0;
}
