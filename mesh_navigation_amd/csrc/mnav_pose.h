// mnav_pose.h -- mesh_map::calculatePoseFromPosition (mesh_map/src/util.cpp:267-298), written once: the device's source
// (k_plan_poses, k_walk_poses of mnav_plans.h) and the host mirror's (tests/test_plans_model.py compiles it with g++).
// The pose at `current` looks at `next` with `normal` up: the basis ex / ey / ez is built in float (lvr2::BaseVector<float>
// component operations, correctly rounded sqrt and division, no contraction), widened to double, turned into a quaternion by
// the published Bullet / tf2 Matrix3x3::getRotation (one sqrt per branch) and divided by its length (:278).  The return
// value is the float length of next - current (:296), the step that makePlan adds to its cost.
// A zero direction, or one parallel to the normal, makes ey = 0 / 0: the quaternion is NaN (position and length are not),
// as in the reference.
#pragma once
#include <cmath>
#include <cstdint>

#include "mnav_walk.h"

namespace mnav {

// tf2::Matrix3x3::getRotation over the basis whose columns are ex, ey, ez, then Quaternion::normalize.  The four branches
// are spelled out (no array indexed by the branch): every value stays in a register on the device.
// branch: 0 trace > 0, 1 / 2 / 3 = the largest diagonal element is xx / yy / zz.
MNAV_HD int pose_basis_quat(double xx, double xy, double xz, double yx, double yy, double yz, double zx, double zy, double zz, double q[4])
{
  // m[r][c]: row r = (ex.r, ey.r, ez.r); here xx = m[0][0], xy = m[0][1], xz = m[0][2], yx = m[1][0], ...
  const double trace = xx + yy + zz;
  double tx, ty, tz, tw;
  int branch;
  if (trace > 0.0) {
    double s = sqrt(trace + 1.0);
    tw = s * 0.5; s = 0.5 / s;
    tx = (zy - yz) * s;
    ty = (xz - zx) * s;
    tz = (yx - xy) * s;
    branch = 0;
  } else if (xx < yy ? yy < zz : xx < zz) {                           // i = 2, j = 0, k = 1
    double s = sqrt(zz - xx - yy + 1.0);
    tz = s * 0.5; s = 0.5 / s;
    tw = (yx - xy) * s;
    tx = (xz + zx) * s;
    ty = (yz + zy) * s;
    branch = 3;
  } else if (xx < yy) {                                               // i = 1, j = 2, k = 0
    double s = sqrt(yy - zz - xx + 1.0);
    ty = s * 0.5; s = 0.5 / s;
    tw = (xz - zx) * s;
    tz = (zy + yz) * s;
    tx = (xy + yx) * s;
    branch = 2;
  } else {                                                            // i = 0, j = 1, k = 2
    double s = sqrt(xx - yy - zz + 1.0);
    tx = s * 0.5; s = 0.5 / s;
    tw = (zy - yz) * s;
    ty = (yx + xy) * s;
    tz = (zx + xz) * s;
    branch = 1;
  }
  const double len = sqrt(tx * tx + ty * ty + tz * tz + tw * tw);
  q[0] = tx / len; q[1] = ty / len; q[2] = tz / len; q[3] = tw / len;
  return branch;
}

// the float length of next - current alone (:295-296)
MNAV_HD float pose_step_length(W3 current, W3 next) { return w3_length(w3_sub(next, current)); }

// pose = { current.x, .y, .z, qx, qy, qz, qw }; *branch_out (optional): the branch of pose_basis_quat
MNAV_HD float pose_from_position(W3 current, W3 next, W3 normal, double pose[7], int* branch_out = nullptr)
{
  const W3 direction = w3_sub(next, current);                         // :295
  const float length = w3_length(direction);                          // :296
  const W3 ez = w3_normalized(normal);                                // :269
  const W3 ey = w3_normalized(w3_cross(normal, direction));           // :270
  const W3 ex = w3_normalized(w3_cross(ey, normal));                  // :271
  double q[4];
  const int branch = pose_basis_quat(ex.x, ey.x, ez.x, ex.y, ey.y, ez.y, ex.z, ey.z, ez.z, q);   // :273, :278-279
  pose[0] = current.x; pose[1] = current.y; pose[2] = current.z;      // :275, :280
  pose[3] = q[0]; pose[4] = q[1]; pose[5] = q[2]; pose[6] = q[3];
  if (branch_out) *branch_out = branch;
  return length;
}

}  // namespace mnav
