// Driver of hgs_hip::LoopMatcherHIP::match_groups (adapters/loop_match_hip.hpp): the candidates of several new keyframes of one graph update
// (LoopDetector::detect, loop_detector.hpp:57-68) through one grouped call, against match() per group on a second matcher.
//   loop_groups_main <method> <n_engines> <max_range> <guesses.bin> T:<keyframe id>:<cloud.bin> C:<keyframe id>:<cloud.bin> ... T:... C:...
// A T token opens a group (its target), every C token behind it is a candidate of that group; guesses.bin holds 16 floats (column-major) per candidate in
// token order; the clouds are pcl::PointXYZI records (32 bytes).  Prints, for match_groups ("G") and then for match per group ("S"), one line per group —
// "best <group> <index>" — and one per record — "<group> <index> <the hgs_result as hex>" —, and at the end "mismatches <n>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <string>
#include <vector>

#include "../../adapters/loop_match_hip.hpp"

static std::vector<char> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) {
    std::fprintf(stderr, "cannot read %s\n", path.c_str());
    std::exit(2);
  }
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void print(const char* tag, const std::vector<std::vector<hgs_result>>& records, const std::vector<int>& best) {
  for (size_t g = 0; g < records.size(); g++) {
    std::printf("%s best %zu %d\n", tag, g, best[g]);
    for (size_t i = 0; i < records[g].size(); i++) {
      std::printf("%s %zu %zu ", tag, g, i);
      const unsigned char* b = reinterpret_cast<const unsigned char*>(&records[g][i]);
      for (size_t k = 0; k < sizeof(hgs_result); k++) std::printf("%02x", b[k]);
      std::printf("\n");
    }
  }
}

int main(int argc, char** argv) {
  if (argc < 7) {
    std::fprintf(stderr, "usage: loop_groups_main <method> <n_engines> <max_range> <guesses.bin> T:<id>:<cloud.bin> C:<id>:<cloud.bin> ...\n");
    return 2;
  }
  const int method = std::atoi(argv[1]), n_engines = std::atoi(argv[2]);
  const double max_range = std::atof(argv[3]);
  const std::vector<char> guesses = slurp(argv[4]);
  std::map<long, std::vector<char>> clouds;  // by keyframe id (node addresses are stable)
  using Matcher = hgs_hip::LoopMatcherHIP;
  std::vector<Matcher::Group> groups;
  size_t n_cand = 0;
  for (int i = 5; i < argc; i++) {
    const std::string tok = argv[i];
    const size_t c1 = tok.find(':'), c2 = tok.find(':', c1 + 1);
    if (c1 != 1 || c2 == std::string::npos || (tok[0] != 'T' && tok[0] != 'C') || (tok[0] == 'C' && groups.empty())) {
      std::fprintf(stderr, "bad token %s\n", tok.c_str());
      return 2;
    }
    const long id = std::atol(tok.substr(c1 + 1, c2 - c1 - 1).c_str());
    if (!clouds.count(id)) clouds[id] = slurp(tok.substr(c2 + 1));
    const std::vector<char>& pts = clouds[id];
    if (tok[0] == 'T') {
      groups.push_back(Matcher::Group{id, pts.data(), pts.size() / 32, 32, {}});
    } else {
      Matcher::Candidate c{id, pts.data(), pts.size() / 32, 32, {}};
      if ((n_cand + 1) * 64 > guesses.size()) {
        std::fprintf(stderr, "guesses.bin is too short\n");
        return 2;
      }
      std::memcpy(c.guess, guesses.data() + n_cand * 64, 64);
      n_cand++;
      groups.back().candidates.push_back(c);
    }
  }
  hgs_params p;
  hgs_params_default(method, &p);
  std::vector<int> devices(n_engines, 0);
  std::vector<std::vector<hgs_result>> rec_g, rec_s(groups.size());
  std::vector<int> best_g, best_s(groups.size(), -1);
  {
    Matcher grouped(p, devices);
    if (!grouped.match_groups(groups, max_range, &rec_g, &best_g)) {
      std::fprintf(stderr, "match_groups failed: %s\n", grouped.last_error().c_str());
      return 1;
    }
  }
  {
    Matcher single(p, devices);
    for (size_t g = 0; g < groups.size(); g++) {
      best_s[g] = single.match(groups[g].points, groups[g].n, groups[g].stride_bytes, groups[g].candidates, max_range, &rec_s[g]);
      if (single.failed_engines() > 0) {
        std::fprintf(stderr, "match failed: %s\n", single.last_error().c_str());
        return 1;
      }
    }
  }
  print("G", rec_g, best_g);
  print("S", rec_s, best_s);
  size_t mismatches = 0;
  for (size_t g = 0; g < groups.size(); g++) {
    mismatches += best_g[g] != best_s[g] || rec_g[g].size() != rec_s[g].size();
    for (size_t i = 0; i < rec_g[g].size() && i < rec_s[g].size(); i++) mismatches += std::memcmp(&rec_g[g][i], &rec_s[g][i], sizeof(hgs_result)) != 0;
  }
  std::printf("mismatches %zu\n", mismatches);
  return mismatches == 0 ? 0 : 1;
}
