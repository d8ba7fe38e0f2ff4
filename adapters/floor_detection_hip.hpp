// floor_detection_hip.hpp — header-only binding of FloorDetectionNodelet::detect (apps/floor_detection_nodelet.cpp:110-180) to hgs_detect_floor:
// height clip, normal filter, RANSAC plane and the acceptance tests run on the device in one call.  The members are the nodelet's parameters
// (initialize_params, :56-66) under their rosparam names; the constants the nodelet hard-codes (k = 10 of :219, the distance threshold 0.1 of :140,
// pcl::SampleConsensus' 1000 iterations and probability 0.99) and the seed of the hypothesis generator sit beside them.
//
// The nodelet's input is the prefilter's output (/filtered_points, :44).  When PrefilteringNodelet::cloud_callback runs in the same process through
// adapters/resident_clouds_hip.hpp, that output is still resident on the device and is used as it is — no second upload; any other cloud is uploaded.
// detect() returns false both when no floor was detected (reason() tells why) and when the device path could not run (device_ran() is false then and
// the caller falls through to the CPU code, the rule of every binding in adapters/).
//
// Deviations from PCL are listed in include/hgs_registration.h (hgs_detect_floor) and DESIGN.md section 11.
#pragma once

#include <Eigen/Dense>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include "hgs_registration.h"
#include "resident_clouds_hip.hpp"

namespace hgs_hip {

template <typename PointT>
class FloorDetector {
public:
  // rosparams of :57-63
  double tilt_deg = 0.0;
  double sensor_height = 2.0;
  double height_clip_range = 1.0;
  int floor_pts_thresh = 512;
  double floor_normal_thresh = 10.0;
  bool use_normal_filtering = true;
  double normal_filter_thresh = 20.0;
  // constants of the reference
  int normal_k = 10;
  double ransac_distance_threshold = 0.1;
  int ransac_max_iterations = 1000;
  double ransac_probability = 0.99;
  uint32_t seed = 0;

  FloorDetector() { ResidentCloudsHIP<PointT>::instance().keepPrefiltered(true); }

  hgs_floor_params params() const {
    hgs_floor_params p;
    hgs_floor_params_default(&p);
    p.tilt_deg = tilt_deg, p.sensor_height = sensor_height, p.height_clip_range = height_clip_range;
    p.floor_pts_thresh = floor_pts_thresh, p.floor_normal_thresh = floor_normal_thresh;
    p.use_normal_filtering = use_normal_filtering ? 1 : 0, p.normal_filter_thresh = normal_filter_thresh;
    p.normal_k = normal_k, p.ransac_distance_threshold = ransac_distance_threshold, p.ransac_max_iterations = ransac_max_iterations;
    p.ransac_probability = ransac_probability, p.seed = seed;
    return p;
  }

  // boost::optional<Eigen::Vector4f> detect(cloud) of :110: true and `coeffs` = the floor plane (normal upward) when a floor was detected.
  // filtered / inliers (null ok): what floor_filtered_pub / floor_points_pub publish.
  bool detect(const pcl::PointCloud<PointT>& cloud, Eigen::Vector4f& coeffs, pcl::PointCloud<PointT>* filtered = nullptr, pcl::PointCloud<PointT>* inliers = nullptr) {
    last_ = hgs_floor_result{};
    const hgs_floor_params p = params();
    device_ran_ = ResidentCloudsHIP<PointT>::instance().detect_floor(cloud, p, &last_, filtered, inliers);
    if (!device_ran_ || !last_.detected) return false;
    for (int i = 0; i < 4; i++) coeffs[i] = last_.coeffs[i];
    return true;
  }

  bool device_ran() const { return device_ran_; }
  int reason() const { return last_.reason; }  // hgs_floor_reason
  const hgs_floor_result& lastResult() const { return last_; }

private:
  hgs_floor_result last_{};
  bool device_ran_ = false;
};

}  // namespace hgs_hip
