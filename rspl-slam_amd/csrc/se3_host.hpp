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

}  // namespace se3h
}  // namespace rspl
