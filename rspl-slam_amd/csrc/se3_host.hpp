// Host-side SE3Quat (g2o): what the handles need to turn the caller's T_wc into the solvers' T_cw estimate
// and back (rspl_frame_optimize, rspl_ba_local).  The device twin is se3_device.hpp.
#pragma once
#include <cmath>

namespace rspl {
namespace se3h {

struct Se3h {  // host SE3Quat (w x y z, t)
  double q[4], t[3];
};

inline void q_to_R(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
  R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

inline void normalize(Se3h& T) {  // SE3Quat::normalizeRotation
  if (T.q[0] < 0)
    for (double& v : T.q) v = -v;
  const double n = std::sqrt(T.q[0] * T.q[0] + T.q[1] * T.q[1] + T.q[2] * T.q[2] + T.q[3] * T.q[3]);
  for (double& v : T.q) v /= n;
}

inline Se3h inverse(const Se3h& T) {  // SE3Quat::inverse
  Se3h r;
  r.q[0] = T.q[0]; r.q[1] = -T.q[1]; r.q[2] = -T.q[2]; r.q[3] = -T.q[3];
  double R[9];
  q_to_R(r.q, R);
  for (int i = 0; i < 3; i++) r.t[i] = -(R[3 * i] * T.t[0] + R[3 * i + 1] * T.t[1] + R[3 * i + 2] * T.t[2]);
  normalize(r);
  return r;
}

// The caller's pose (q: x y z w, p; T_wc) to the solver's estimate T[8] (T_cw: q w x y z, t, pad) --
// VertexSE3Expmap estimate = SE3Quat(q, p).inverse() (g2o_optimization.cc:42) -- and back: T_wc =
// estimate().inverse() (:235-240)
inline void pose_to_estimate(const double* q_xyzw, const double* p, double* T) {
  Se3h Twc;
  Twc.q[0] = q_xyzw[3];
  Twc.q[1] = q_xyzw[0];
  Twc.q[2] = q_xyzw[1];
  Twc.q[3] = q_xyzw[2];
  for (int k = 0; k < 3; k++) Twc.t[k] = p[k];
  normalize(Twc);
  const Se3h Tcw = inverse(Twc);
  for (int k = 0; k < 4; k++) T[k] = Tcw.q[k];
  for (int k = 0; k < 3; k++) T[4 + k] = Tcw.t[k];
  T[7] = 0;
}
inline void estimate_to_pose(const double* T, double* q_xyzw, double* p) {
  Se3h Tcw;
  for (int k = 0; k < 4; k++) Tcw.q[k] = T[k];
  for (int k = 0; k < 3; k++) Tcw.t[k] = T[4 + k];
  const Se3h Twc = inverse(Tcw);
  q_xyzw[0] = Twc.q[1];
  q_xyzw[1] = Twc.q[2];
  q_xyzw[2] = Twc.q[3];
  q_xyzw[3] = Twc.q[0];
  for (int k = 0; k < 3; k++) p[k] = Twc.t[k];
}

}  // namespace se3h
}  // namespace rspl
