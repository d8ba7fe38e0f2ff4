// Driver of hgs_hip::ResidentCloudsHIP::fitness_scores (adapters/resident_clouds_hip.hpp): the fitness scores of all edges of one graph update
// (flush_keyframe_queue and the loop step, apps/hdl_graph_slam_nodelet.cpp:235,569) through one batched call, against fitness_score per pair on a second
// instance.
//   edge_fitness_main <max_range> <poses.bin> C:<cloud id>:<cloud.bin> ... P:<cloud1 id>:<cloud2 id> ...
// poses.bin holds 16 floats (column-major) per P token in token order; the clouds are pcl::PointXYZI records (32 bytes).  Prints one line per pair for the
// batch — "B <pair> <score as a hex double>" — and one for the per-pair calls — "S <pair> <score>" —, the device calls each side made, and at the end
// "mismatches <n>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../adapters/resident_clouds_hip.hpp"

using Clouds = hgs_hip::ResidentCloudsHIP<pcl::PointXYZI>;

static std::vector<char> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) {
    std::fprintf(stderr, "cannot read %s\n", path.c_str());
    std::exit(2);
  }
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: edge_fitness_main <max_range> <poses.bin> C:<id>:<cloud.bin> ... P:<id1>:<id2> ...\n");
    return 2;
  }
  const double max_range = std::atof(argv[1]);
  const std::vector<char> poses = slurp(argv[2]);
  std::map<long, Clouds::CloudConstPtr> clouds;
  std::vector<Clouds::EdgePair> pairs;
  for (int i = 3; i < argc; i++) {
    const std::string tok = argv[i];
    const size_t c1 = tok.find(':'), c2 = tok.find(':', c1 + 1);
    if (c1 != 1 || c2 == std::string::npos || (tok[0] != 'C' && tok[0] != 'P')) {
      std::fprintf(stderr, "bad token %s\n", tok.c_str());
      return 2;
    }
    const long id = std::atol(tok.substr(c1 + 1, c2 - c1 - 1).c_str());
    if (tok[0] == 'C') {
      const std::vector<char> bytes = slurp(tok.substr(c2 + 1));
      auto cloud = std::make_shared<Clouds::Cloud>();
      cloud->points.resize(bytes.size() / sizeof(pcl::PointXYZI));
      if (!bytes.empty()) std::memcpy(static_cast<void*>(cloud->points.data()), bytes.data(), cloud->points.size() * sizeof(pcl::PointXYZI));
      clouds[id] = cloud;
      continue;
    }
    const long id2 = std::atol(tok.substr(c2 + 1).c_str());
    if (!clouds.count(id) || !clouds.count(id2) || (pairs.size() + 1) * 64 > poses.size()) {
      std::fprintf(stderr, "pair %s names an unknown cloud, or poses.bin is too short\n", tok.c_str());
      return 2;
    }
    Clouds::EdgePair p;
    p.cloud1 = clouds[id], p.cloud2 = clouds[id2];
    std::memcpy(p.relpose, poses.data() + pairs.size() * 64, 64);
    pairs.push_back(p);
  }
  std::vector<double> batch, single(pairs.size(), 0.0);
  size_t calls_batch = 0, calls_single = 0;
  {
    Clouds dev;
    if (!dev.fitness_scores(pairs, max_range, &batch)) {
      std::fprintf(stderr, "fitness_scores failed: %s\n", dev.last_error().c_str());
      return 1;
    }
    calls_batch = dev.device_calls();
  }
  {
    Clouds dev;
    for (size_t i = 0; i < pairs.size(); i++)
      if (!dev.fitness_score(pairs[i].cloud1, pairs[i].cloud2, pairs[i].relpose, max_range, &single[i])) {
        std::fprintf(stderr, "fitness_score failed: %s\n", dev.last_error().c_str());
        return 1;
      }
    calls_single = dev.device_calls();
  }
  size_t mismatches = batch.size() != single.size();
  for (size_t i = 0; i < batch.size(); i++) std::printf("B %zu %a\n", i, batch[i]);
  for (size_t i = 0; i < single.size(); i++) std::printf("S %zu %a\n", i, single[i]);
  for (size_t i = 0; i < batch.size() && i < single.size(); i++) mismatches += std::memcmp(&batch[i], &single[i], sizeof(double)) != 0;
  std::printf("device_calls batch %zu single %zu\n", calls_batch, calls_single);
  std::printf("mismatches %zu\n", mismatches);
  return mismatches == 0 ? 0 : 1;
}
