// TEST ONLY — the patched hdl_graph_slam::select_registration_method (src/hdl_graph_slam/registrations.cpp + integration/hdl_graph_slam_hip.patch)
// for registration_method = ICP_HIP: the object it returns and the engine parameters the rosparams turned into; plain ICP for comparison.
// Usage: icp_factory_main   (no arguments; nothing runs on a device)
#include <cstdio>
#include <string>
#include <hdl_graph_slam/registrations.hpp>
#include <registration_hip.hpp>

using PointT = pcl::PointXYZI;

int main() {
  struct Case {
    const char* method;
    const char* reciprocal;  // nullptr: rosparam not set
  } cases[] = {{"ICP_HIP", nullptr}, {"ICP_HIP", "true"}, {"ICP", nullptr}};
  for (const Case& c : cases) {
    ros::NodeHandle pnh;
    pnh.params["registration_method"] = c.method;
    if (c.reciprocal) {
      pnh.params["reg_use_reciprocal_correspondences"] = c.reciprocal;
      pnh.params["reg_max_correspondence_distance"] = "1.5";
      pnh.params["reg_maximum_iterations"] = "32";
      pnh.params["reg_transformation_epsilon"] = "0.001";
    }
    auto registration = hdl_graph_slam::select_registration_method(pnh);
    auto* hip = dynamic_cast<hgs_hip::RegistrationHIP<PointT, PointT>*>(registration.get());
    std::printf("%s hip %d", c.method, hip ? 1 : 0);
    if (hip) {
      const hgs_params& p = hip->params();
      std::printf(" method %d max_iterations %d transformation_epsilon %.17g rotation_epsilon %.17g max_correspondence_distance %.17g reciprocal %d", p.method,
                  p.max_iterations, p.transformation_epsilon, p.rotation_epsilon, p.max_correspondence_distance, p.icp_reciprocal);
    }
    std::printf("\n");
  }
  return 0;
}
