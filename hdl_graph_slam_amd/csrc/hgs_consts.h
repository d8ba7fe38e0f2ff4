// hgs_consts.h — how the public parameters (include/hgs_registration.h) map onto the constants the kernels take (host only).  One copy: the engine
// and the host emulation that checks it (tests/emul/emul.cpp) both include this file.
#pragma once
#include <cfloat>
#include <cmath>

#include "../../include/hgs_registration.h"
#include "hgs_floor.h"
#include "hgs_gicp.h"
#include "hgs_icp.h"
#include "hgs_ndt.h"
#include "hgs_vgicp.h"

namespace hgs {

inline GicpConsts gicp_consts(const hgs_params& p) {
  GicpConsts c;
  const double thr = p.max_correspondence_distance;
  c.max_corr2 = thr * thr;
  c.search_bound2 = c.max_corr2 >= (double)FLT_MAX ? FLT_MAX : nextafterf((float)c.max_corr2, FLT_MAX);
  c.rotation_eps = p.rotation_epsilon;
  c.translation_eps = p.transformation_epsilon;
  c.lm_init_lambda_factor = p.lm_init_lambda_factor;
  c.lm_max_iterations = p.lm_max_iterations;
  c.max_iterations = p.max_iterations;
  c.k_correspondences = p.correspondence_randomness;
  return c;
}

inline VgicpConsts vgicp_consts(const hgs_params& p) {
  VgicpConsts c;
  c.resolution = p.resolution;
  c.search = p.neighbor_search == HGS_DIRECT27 ? 3 : (p.neighbor_search == HGS_DIRECT7 ? 2 : 1);
  c.pad = 0;
  return c;
}

// pcl::IterativeClosestPoint as registrations.cpp:57-64 configures it, with DefaultConvergenceCriteria's thresholds (hgs_icp.h)
inline IcpConsts icp_consts(const hgs_params& p) {
  IcpConsts c;
  const double thr = p.max_correspondence_distance;
  c.max_corr2 = thr * thr;
  c.search_bound2 = c.max_corr2 >= (double)FLT_MAX ? FLT_MAX : nextafterf((float)c.max_corr2, FLT_MAX);
  c.max_iterations = p.max_iterations;
  c.trans_eps = p.transformation_epsilon;
  c.rot_thr = p.rotation_epsilon > 0 ? p.rotation_epsilon : 1.0 - p.transformation_epsilon;
  c.reciprocal = p.icp_reciprocal ? 1 : 0;
  c.pad = 0;
  return c;
}

// (pad = 1 asks the kernels for a device-side per-iteration trace: the engine sets it at its call sites, nothing here reads the environment)
inline NdtConsts ndt_consts(const hgs_params& p) {
  NdtConsts c;
  const double c1 = 10.0 * (1 - p.ndt_outlier_ratio);
  const double c2 = p.ndt_outlier_ratio / std::pow(p.resolution, 3);
  const double d3 = -std::log(c2);
  c.gauss_d1 = -std::log(c1 + c2) - d3;
  c.gauss_d2 = -2 * std::log((-std::log(c1 * std::exp(-0.5) + c2) - d3) / c.gauss_d1);
  c.step_size = p.ndt_step_size;
  c.trans_eps = p.transformation_epsilon;
  c.max_iterations = p.max_iterations;
  c.search = p.neighbor_search == HGS_DIRECT1 ? 1 : (p.neighbor_search == HGS_KDTREE ? 0 : 2);
  c.kdtree_radius2 = (float)(p.resolution * p.resolution);
  c.line_search = p.ndt_line_search ? 1 : 0;
  c.upstream_hd1_sign = p.ndt_upstream_hd1_sign;
  c.pad = 0;
  return c;
}

inline FloorConsts floor_consts(const hgs_floor_params* p) {
  FloorConsts c{};
  // tilt_matrix (:112-113): the angle is a float (Eigen::AngleAxisf); z' = (R p).z = -sin * x + cos * z, r = R^-1 e_z = (-sin, 0, cos)
  const double angle = (double)(float)(p->tilt_deg * M_PI / 180.0);
  c.rx = p->tilt_deg == 0.0 ? 0.f : -(float)std::sin(angle);
  c.rz = p->tilt_deg == 0.0 ? 1.f : (float)std::cos(angle);
  c.nrx = (double)c.rx, c.nrz = (double)c.rz;
  c.clip_lo = (float)(p->sensor_height + p->height_clip_range);  // :118
  c.clip_hi = (float)(p->sensor_height - p->height_clip_range);  // :119
  c.normal_cos = std::cos(p->normal_filter_thresh * M_PI / 180.0);  // :228
  c.dist_thresh = p->ransac_distance_threshold;
  c.log_prob = std::log(1.0 - p->ransac_probability);
  c.max_iterations = p->ransac_max_iterations;
  c.seed = p->seed;
  return c;
}

}  // namespace hgs
