// TEST ONLY — adapters/registration_hip.hpp as the ICP_HIP branch of the patched factory builds it: construct with HGS_ICP,
// the setters of registrations.cpp:57-64, then driven like a pcl::Registration through the base pointer.
// Usage: icp_adapter_main <reciprocal 0|1> <target.bin> <source.bin>   (raw PointXYZI records)
// Prints: the class name, the engine parameters, converged / iterations / passes and the final transform (column-major).
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <pcl/point_types.h>
#include "../../adapters/registration_hip.hpp"

using PointT = pcl::PointXYZI;

// reg_name_ is a protected member of pcl::Registration (getClassName() in PCL)
struct NamedICP : hgs_hip::RegistrationHIP<PointT, PointT> {
  using hgs_hip::RegistrationHIP<PointT, PointT>::RegistrationHIP;
  const std::string& name() const { return this->reg_name_; }
};

static pcl::PointCloud<PointT>::Ptr load(const char* path) {
  auto c = std::make_shared<pcl::PointCloud<PointT>>();
  FILE* f = std::fopen(path, "rb");
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  PointT p;
  while (std::fread(&p, sizeof(PointT), 1, f) == 1) c->points.push_back(p);
  std::fclose(f);
  return c;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s reciprocal target.bin source.bin\n", argv[0]);
    return 2;
  }
  try {
    auto icp = std::make_shared<NamedICP>(HGS_ICP, 0);
    icp->setTransformationEpsilon(0.01);
    icp->setMaximumIterations(64);
    icp->setMaxCorrespondenceDistance(2.5);
    icp->setUseReciprocalCorrespondences(std::atoi(argv[1]) != 0);
    const hgs_params& p = icp->params();
    std::printf("name %s\n", icp->name().c_str());
    std::printf("params %d %d %.17g %.17g %.17g %d\n", p.method, p.max_iterations, p.transformation_epsilon, p.rotation_epsilon, p.max_correspondence_distance,
                p.icp_reciprocal);
    pcl::Registration<PointT, PointT>::Ptr registration = icp;
    registration->setInputTarget(load(argv[2]));
    registration->setInputSource(load(argv[3]));
    pcl::PointCloud<PointT> aligned;
    registration->align(aligned, pcl::MockMatrix4f::Identity());
    std::printf("converged %d iterations %d passes %d\n", (int)registration->hasConverged(), icp->lastResult().iterations, icp->lastResult().lm_tries);
    const auto T = registration->getFinalTransformation();
    for (int i = 0; i < 16; i++) std::printf("%.9g ", T.data()[i]);
    std::printf("\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
