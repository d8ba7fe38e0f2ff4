// hgs_icp.h — point-to-point ICP: the per-point arithmetic and the per-problem control step of
// pcl::IterativeClosestPoint<PointXYZI, PointXYZI> as the factory configures it (src/hdl_graph_slam/registrations.cpp:57-64):
// exact 1-NN correspondences (optionally reciprocal), a closed-form Umeyama step without scale (PCL's default
// TransformationEstimationSVD) and PCL's DefaultConvergenceCriteria.  The test-side restatement is tests/icp_reference.py.
// HGS_HD: the HIP kernels call these; the test-only host harness (tests/emul) compiles the very same functions.
#pragma once
#include "hgs_math.h"

namespace hgs {

// Sums of one correspondence pass (k_icp_correspond, per tile; k_icp_solve, per problem):
// [0] pairs, [1..3] sum p, [4..6] sum q, [7..15] sum q p^T (row-major: row = target coordinate, column = source coordinate), [16] sum d2.
// p is the moved source point as it was searched (float), q its target point (float): every product is exact in double.
constexpr int kAccIcp = 17;

struct IcpConsts {
  double max_corr2;     // max_correspondence_distance^2; a pair is kept when (double)d2 <= max_corr2 (PCL; fast_gicp's GICP uses <)
  float search_bound2;  // float upper bound handed to the tree search (>= max_corr2)
  int max_iterations;
  double trans_eps;     // translation threshold: compared with the SQUARED translation of the step (DefaultConvergenceCriteria)
  double rot_thr;       // cos(angle) threshold: rotation_epsilon if > 0, else 1 - transformation_epsilon
  int reciprocal;       // setUseReciprocalCorrespondences
  int pad;
};

enum IcpPhase { ICP_RUN = 0, ICP_DONE = 2 };

struct IcpState {
  Pose x;           // final_transformation_
  double mse;       // mean d2 of the last iteration's correspondences (the result's `error`; DBL_MAX before the first iteration)
  double mse_prev;  // DefaultConvergenceCriteria::correspondences_prev_mse_ (DBL_MAX at the start of every registration)
  int phase;
  int iterations;   // nr_iterations_
  int passes;       // correspondence passes (the result's lm_tries)
  int converged;
};

HGS_HD void icp_state_init(IcpState& s, const float* guess_colmajor) {
  s.x = pose_from_colmajor_f(guess_colmajor);
  s.mse = DBL_MAX, s.mse_prev = DBL_MAX;
  s.phase = ICP_RUN;
  s.iterations = 0, s.passes = 0, s.converged = 0;
}

// The source point moved by the current pose: pose in double, unfused, in this order, rounded to float — the query the search
// sees (tests/icp_reference.py evaluates the same expression tree with numpy).
HGS_HD F3 icp_move_point(const Pose& T, float ax, float ay, float az) {
  HGS_FP_STRICT
  const double x = (double)ax, y = (double)ay, z = (double)az;
  F3 q;
  q.x = (float)(((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3]);
  q.y = (float)(((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7]);
  q.z = (float)(((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11]);
  return q;
}
// A target point taken back into the source frame, T^-1 q = R^T (q - t): the query of the reciprocal search in the source's own index.
HGS_HD F3 icp_unmove_point(const Pose& T, float qx, float qy, float qz) {
  HGS_FP_STRICT
  const double x = (double)qx - T.m[3], y = (double)qy - T.m[7], z = (double)qz - T.m[11];
  F3 p;
  p.x = (float)((T.m[0] * x + T.m[4] * y) + T.m[8] * z);
  p.y = (float)((T.m[1] * x + T.m[5] * y) + T.m[9] * z);
  p.z = (float)((T.m[2] * x + T.m[6] * y) + T.m[10] * z);
  return p;
}

// One pair's terms in accumulator order.
HGS_HD void icp_pair_terms(const F3& p, float qx, float qy, float qz, float d2, double* t /*[kAccIcp]*/) {
  const double px = p.x, py = p.y, pz = p.z, tx = qx, ty = qy, tz = qz;
  t[0] = 1.0;
  t[1] = px, t[2] = py, t[3] = pz;
  t[4] = tx, t[5] = ty, t[6] = tz;
  t[7] = tx * px, t[8] = tx * py, t[9] = tx * pz;
  t[10] = ty * px, t[11] = ty * py, t[12] = ty * pz;
  t[13] = tz * px, t[14] = tz * py, t[15] = tz * pz;
  t[16] = (double)d2;
}

// SVD of a 3x3 matrix (row-major): A = U diag(s) V^T, s descending.  One-sided Jacobi on the columns of A V (svd6_rotate's
// rotation), then the columns normalised; a (numerically) zero singular direction is completed to a right-handed basis —
// the rotation below does not depend on its sign.
HGS_HD void svd3(const double* A, double* U, double* s, double* V) {
  HGS_FP_STRICT
  double B[9];
  for (int i = 0; i < 9; i++) B[i] = A[i], V[i] = (i % 4 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 32; sweep++) {
    bool rotated = false;
    for (int pair = 0; pair < 3; pair++) {
      const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2;
      double alpha = 0, beta = 0, gamma = 0;
      for (int k = 0; k < 3; k++) {
        alpha += B[k * 3 + p] * B[k * 3 + p];
        beta += B[k * 3 + q] * B[k * 3 + q];
        gamma += B[k * 3 + p] * B[k * 3 + q];
      }
      if (gamma == 0.0 || fabs(gamma) <= DBL_EPSILON * sqrt(alpha * beta)) continue;
      const double zeta = (beta - alpha) / (2.0 * gamma);
      const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
      for (int k = 0; k < 3; k++) {
        const double bp = B[k * 3 + p], bq = B[k * 3 + q], vp = V[k * 3 + p], vq = V[k * 3 + q];
        B[k * 3 + p] = c * bp - sn * bq, B[k * 3 + q] = sn * bp + c * bq;
        V[k * 3 + p] = c * vp - sn * vq, V[k * 3 + q] = sn * vp + c * vq;
      }
      rotated = true;
    }
    if (!rotated) break;
  }
  int order[3] = {0, 1, 2};
  double nrm[3];
  for (int j = 0; j < 3; j++) nrm[j] = sqrt(B[j] * B[j] + B[3 + j] * B[3 + j] + B[6 + j] * B[6 + j]);
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 2 - i; j++)
      if (nrm[order[j]] < nrm[order[j + 1]]) {
        const int o = order[j];
        order[j] = order[j + 1], order[j + 1] = o;
      }
  double Vs[9];
  for (int j = 0; j < 3; j++) {
    const int o = order[j];
    s[j] = nrm[o];
    for (int k = 0; k < 3; k++) Vs[k * 3 + j] = V[k * 3 + o], U[k * 3 + j] = s[j] > 0.0 ? B[k * 3 + o] / s[j] : 0.0;
  }
  for (int i = 0; i < 9; i++) V[i] = Vs[i];
  const double tiny = s[0] * 1e-13;
  if (!(s[0] > 0.0)) {  // A = 0: any basis
    for (int i = 0; i < 9; i++) U[i] = (i % 4 == 0) ? 1.0 : 0.0;
    return;
  }
  if (!(s[1] > tiny)) {  // rank 1: a unit vector orthogonal to u0
    const double ax = fabs(U[0]), ay = fabs(U[3]), az = fabs(U[6]);
    const double e[3] = {ax <= ay && ax <= az ? 1.0 : 0.0, ay < ax && ay <= az ? 1.0 : 0.0, az < ax && az < ay ? 1.0 : 0.0};
    double w[3] = {U[3] * e[2] - U[6] * e[1], U[6] * e[0] - U[0] * e[2], U[0] * e[1] - U[3] * e[0]};
    const double wn = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    for (int k = 0; k < 3; k++) U[k * 3 + 1] = w[k] / wn;
  }
  if (!(s[2] > tiny)) {  // rank <= 2: u2 = u0 x u1
    U[2] = U[3] * U[7] - U[6] * U[4];
    U[5] = U[6] * U[1] - U[0] * U[7];
    U[8] = U[0] * U[4] - U[3] * U[1];
  }
}

HGS_HD double det3(const double* M) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// Eigen's umeyama(src, dst, false) from the pass's sums: Sigma = (1/n) sum (q - mu_q)(p - mu_p)^T = U S V^T,
// D = diag(1, 1, det U det V < 0 ? -1 : 1), R = U D V^T, t = mu_q - R mu_p.  Delta row-major 3x4.
HGS_HD void icp_umeyama(const double* acc, Pose& delta) {
  HGS_FP_STRICT
  const double inv = 1.0 / acc[0];
  const double mp[3] = {acc[1] * inv, acc[2] * inv, acc[3] * inv}, mq[3] = {acc[4] * inv, acc[5] * inv, acc[6] * inv};
  double S[9], U[9], sv[3], V[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) S[r * 3 + c] = acc[7 + r * 3 + c] * inv - mq[r] * mp[c];
  svd3(S, U, sv, V);
  const double d = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) delta.m[r * 4 + c] = (U[r * 3 + 0] * V[c * 3 + 0] + U[r * 3 + 1] * V[c * 3 + 1]) + d * U[r * 3 + 2] * V[c * 3 + 2];
  }
  for (int r = 0; r < 3; r++) delta.m[r * 4 + 3] = mq[r] - ((delta.m[r * 4 + 0] * mp[0] + delta.m[r * 4 + 1] * mp[1]) + delta.m[r * 4 + 2] * mp[2]);
}

// One iteration of IterativeClosestPoint::computeTransformation behind a correspondence pass (acc = the pass's sums):
// fewer than 3 pairs -> not converged, stop, pose kept; else the Umeyama step, final = Delta * final, ++iterations, and
// DefaultConvergenceCriteria::hasConverged in its order (max iterations — counts as converged —, transformation, absolute MSE;
// the relative-MSE test is off: euclidean_fitness_epsilon = -DBL_MAX).
HGS_HD void icp_after_pass(IcpState& s, const double* acc, const IcpConsts& c) {
  HGS_FP_STRICT
  s.passes++;
  if (!(acc[0] >= 3.0)) {
    s.converged = 0;
    s.phase = ICP_DONE;
    return;
  }
  const double mse = acc[16] / acc[0];
  Pose delta;
  icp_umeyama(acc, delta);
  s.x = pose_mul(delta, s.x);
  s.iterations++;
  s.mse = mse;
  bool done = s.iterations >= c.max_iterations;
  if (!done) {
    const double cos_angle = 0.5 * (delta.m[0] + delta.m[5] + delta.m[10] - 1.0);
    const double t2 = delta.m[3] * delta.m[3] + delta.m[7] * delta.m[7] + delta.m[11] * delta.m[11];
    done = cos_angle >= c.rot_thr && t2 <= c.trans_eps;
  }
  if (!done) done = fabs(mse - s.mse_prev) < 1e-12;
  if (done) {
    s.converged = 1;
    s.phase = ICP_DONE;
    return;
  }
  s.mse_prev = mse;
}

}  // namespace hgs
