// hgs_floor.h — floor detection: the per-point and per-hypothesis arithmetic and the sequential RANSAC rule of
// FloorDetectionNodelet::detect (apps/floor_detection_nodelet.cpp:110-180): height clip (plane_clip, :189-204), normal filter
// (normal_filtering, :211-238) and pcl::RandomSampleConsensus over pcl::SampleConsensusModelPlane with a distance threshold of 0.1 (:138-141).
// Deviations from PCL: the hypothesis sequence is a counter-based generator of ours (PCL shuffles with a boost::mt19937);
// a degenerate triple counts as an iteration (PCL redraws); plane and distance arithmetic is fp64 (PCL: float); the neighbourhood covariance is
// centred fp64 (PCL: a float covariance whose form differs between PCL versions); with tilt_deg != 0 the filtered points keep the input's own
// bits (PCL rotates there and back in float).  With tilt_deg = 0 the clip is bit-exact PCL.  The test-side restatement is tests/floor_reference.py.
// HGS_HD: the HIP kernels call these; the host emulation of tests/emul compiles the very same functions.
#pragma once
#include "hgs_math.h"

namespace hgs {

struct FloorConsts {
  float rx, rz;            // r = R^-1 e_z = (rx, 0, rz) as floats: rx = -sin(tilt), rz = cos(tilt) of the float angle; z' = (R p).z = rx * x + rz * z
  float clip_lo, clip_hi;  // (float)(sensor_height + height_clip_range), (float)(sensor_height - height_clip_range)
  double nrx, nrz;         // the same direction in double (normal filter: |n . r|)
  double normal_cos;       // cos(normal_filter_thresh)
  double dist_thresh;      // ransac_distance_threshold
  double log_prob;         // log(1 - ransac_probability)
  int max_iterations;      // ransac_max_iterations
  unsigned seed;
};

// the two plane_clip calls (:118-119) with PCL's `distance >= 0` rule, in float: kept between the two planes.  A point with a non-finite
// coordinate is dropped (pcl::transformPointCloud's full matrix product makes its z' NaN).
HGS_HD bool floor_clip_keep(const FloorConsts& c, float x, float y, float z) {
  HGS_FP_STRICT
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
  const float zt = c.rx * x + c.rz * z;
  return (zt + c.clip_lo >= 0.f) && !(zt + c.clip_hi >= 0.f);
}

// pcl::NormalEstimation gives a point with fewer than three neighbours (itself included) a NaN normal (pcl::computePointNormal), and the filter's test
// on NaN fails: of a clipped cloud of fewer than three points the normal filter keeps nothing.  (Two points have a rank-1 covariance, whose smallest
// eigenvector is any direction across the line between them.)
HGS_HD bool floor_normals_defined(size_t n_clipped) { return n_clipped >= 3; }

// unit eigenvector of the smallest eigenvalue of a neighbourhood covariance, and the normal filter's test |n . r| > cos(normal_filter_thresh)
HGS_HD bool floor_normal_keep(const FloorConsts& c, const Sym3& cov, double* n3) {
  HGS_FP_STRICT
  const double A[9] = {cov.xx, cov.xy, cov.xz, cov.xy, cov.yy, cov.yz, cov.xz, cov.yz, cov.zz};
  double w[3], V[9];
  eig_sym3(A, w, V);  // ascending
  double nx = V[0], ny = V[3], nz = V[6];
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  nx /= len, ny /= len, nz /= len;
  n3[0] = nx, n3[1] = ny, n3[2] = nz;
  return fabs(nx * c.nrx + nz * c.nrz) > c.normal_cos;
}

// ---- the hypothesis generator: indices of three distinct points as a pure function of (seed, i, n) ---------------------------
// splitmix64's finaliser; draw j of hypothesis i is mix(mix(seed * 2^32 + i) + (j + 1) * 0x9e3779b97f4a7c15).
HGS_HD unsigned long long floor_mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// a = r0 mod n; b = r1 mod (n - 1), stepped over a; c = r2 mod (n - 2), stepped over the smaller and then the larger of a, b.  n >= 3.
HGS_HD void floor_sample3(unsigned seed, unsigned i, unsigned n, unsigned* a, unsigned* b, unsigned* c) {
  const unsigned long long base = floor_mix64(((unsigned long long)seed << 32) | (unsigned long long)i);
  const unsigned long long r0 = floor_mix64(base + 0x9e3779b97f4a7c15ull), r1 = floor_mix64(base + 2ull * 0x9e3779b97f4a7c15ull),
                           r2 = floor_mix64(base + 3ull * 0x9e3779b97f4a7c15ull);
  const unsigned ia = (unsigned)(r0 % n);
  unsigned ib = (unsigned)(r1 % (n - 1u));
  if (ib >= ia) ib++;
  unsigned ic = (unsigned)(r2 % (n - 2u));
  const unsigned lo = ia < ib ? ia : ib, hi = ia < ib ? ib : ia;
  if (ic >= lo) ic++;
  if (ic >= hi) ic++;
  *a = ia, *b = ib, *c = ic;
}

// the plane through three float points in fp64: n = (p1 - p0) x (p2 - p0) normalised, d = -n . p0; false (all zero) for a degenerate triple
HGS_HD bool floor_plane3(const float4& p0, const float4& p1, const float4& p2, double* pl) {
  HGS_FP_STRICT
  const double ax = (double)p1.x - (double)p0.x, ay = (double)p1.y - (double)p0.y, az = (double)p1.z - (double)p0.z;
  const double bx = (double)p2.x - (double)p0.x, by = (double)p2.y - (double)p0.y, bz = (double)p2.z - (double)p0.z;
  double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  if (!(len > 0.0) || !(len < DBL_MAX)) {
    pl[0] = pl[1] = pl[2] = pl[3] = 0.0;
    return false;
  }
  nx /= len, ny /= len, nz /= len;
  pl[0] = nx, pl[1] = ny, pl[2] = nz;
  pl[3] = -((nx * (double)p0.x + ny * (double)p0.y) + nz * (double)p0.z);
  return true;
}
// |n . p + d| < threshold in fp64 (false for a non-finite point)
HGS_HD bool floor_within(const double* pl, double x, double y, double z, double thresh) {
  HGS_FP_STRICT
  return fabs(((pl[0] * x + pl[1] * y) + pl[2] * z) + pl[3]) < thresh;
}

// ---- the sequential rule of pcl::RandomSampleConsensus::computeModel over the hypotheses' counts -----------------------------------
struct FloorRansacState {
  double k;          // iterations the current best model asks for
  double plane[4];   // the best hypothesis's plane
  int best;          // its count (0: none yet)
  int best_i;        // its index (-1: none)
  int iterations;    // hypotheses evaluated
  int done;
};
HGS_HD void floor_ransac_init(FloorRansacState& s, int max_iterations) {
  s.k = 1.0;
  s.plane[0] = s.plane[1] = s.plane[2] = s.plane[3] = 0.0;
  s.best = 0, s.best_i = -1, s.iterations = 0;
  s.done = max_iterations <= 0 ? 1 : 0;
}
// hypothesis i is evaluated while i < k and i < max_iterations
HGS_HD bool floor_ransac_goes_on(const FloorRansacState& s, int i, int max_iterations) { return (double)i < s.k && i < max_iterations; }
// hypothesis i with `count` points of n within the threshold: a strictly better count becomes the best and sets k = log(1 - p) / log(1 - w^3)
HGS_HD bool floor_ransac_step(FloorRansacState& s, int i, int count, int n, double log_prob) {
  HGS_FP_STRICT
  s.iterations = i + 1;
  if (count <= s.best) return false;
  s.best = count, s.best_i = i;
  const double w = (double)count / (double)n;
  double p_no = 1.0 - (w * w) * w;
  const double eps = 2.220446049250313e-16;  // std::numeric_limits<double>::epsilon(), as PCL clamps
  p_no = p_no > eps ? p_no : eps;
  p_no = p_no < 1.0 - eps ? p_no : 1.0 - eps;
  s.k = log_prob / log(p_no);
  return true;
}

}  // namespace hgs
