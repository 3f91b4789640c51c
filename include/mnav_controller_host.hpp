/* mnav_controller_host.hpp -- the host half of mesh_controller::MeshController, written once.
 *
 * libmnav's two front ends (the ROS 2 plugin package integration/mesh_gpu_planners and its ROS-free twin
 * mesh_navigation_amd/csrc/adapter) both present the reference's controller class.  What that class does around the
 * device tick (mnav_follow_batch, mnav.h) follows the same lines of mesh_controller.cpp in both, so it lives here on plain
 * numbers and is wrapped by both:
 *
 *   FieldFollower::setPlan                  :179-193   goal position / direction, where the field is resident, no current face
 *   FieldFollower::computeVelocityCommands  :67-170    quaternion -> heading and up vector, ONE device call with n = 1,
 *                                                      current_face_ / robot_pos_ kept for the next tick
 *   FieldFollower::isGoalReached            :172-177   on the host, from the kept position and heading
 *   direction_of                            :202-213   tf2's quaternion-to-basis product applied to an axis, in double
 *   SharedContext                           the device context with the lock both plugins take around their calls on it, and
 *                                           a handle that outlives the planner without dangling
 *   publish_field / lookup_field            how a planner plugin tells a controller plugin of the same process (they only share
 *                                           the MeshMap pointer) which context and plan hold the field of its last successful
 *                                           plan; the reference passes the field itself through MeshMap::setVectorMap / getVectorMap
 *
 * Header-only; needs nothing but the C ABI (mnav.h) and the standard library.  Outcomes are named after the constants of
 * mbf_msgs::action::ExePath::Result they stand for; their VALUES are this header's own (the message package is not part
 * of this tree) -- the ROS plugin maps them to the named constants. */
#pragma once

#include <atomic>
#include <cmath>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <string>

#include "mnav.h"

namespace mnav_host {

enum FollowOutcome : uint32_t { FOLLOW_SUCCESS = 0, FOLLOW_OUT_OF_MAP = 1, FOLLOW_FAILURE = 2, FOLLOW_CANCELED = 3, FOLLOW_INTERNAL_ERROR = 4 };

/* mesh_controller.cpp:202-213: tf2::Matrix3x3::setRotation(q) (tf2/LinearMath/Matrix3x3.h) times `axis`, in double; the
 * result is narrowed to float where mesh_map::Normal(v.x(), v.y(), v.z()) does (:212).  Whether that constructor normalises
 * again is lvr2's and not restated. */
inline void direction_of(const double q_xyzw[4], const double axis[3], float out[3])
{
  const double x = q_xyzw[0], y = q_xyzw[1], z = q_xyzw[2], w = q_xyzw[3];
  const double d = x * x + y * y + z * z + w * w;
  const double s = 2.0 / d;
  const double xs = x * s, ys = y * s, zs = z * s;
  const double wx = w * xs, wy = w * ys, wz = w * zs;
  const double xx = x * xs, xy = x * ys, xz = x * zs;
  const double yy = y * ys, yz = y * zs, zz = z * zs;
  const double m[3][3] = { { 1.0 - (yy + zz), xy - wz, xz + wy }, { xy + wz, 1.0 - (xx + zz), yz - wx }, { xz - wy, yz + wx, 1.0 - (xx + yy) } };
  for (int r = 0; r < 3; ++r) out[r] = (float)(m[r][0] * axis[0] + m[r][1] * axis[1] + m[r][2] * axis[2]);
}

/* One device context and the lock that belongs to it.  mnav_ctx itself has no lock and allows one call at a time
 * (INTEGRATION.md section 4); Move Base Flex runs get_path and exe_path at once, so the planner that owns the context takes
 * `mutex` around every device call of makePlan and the controller takes it around its tick: a tick waits for a running
 * plan and the other way round.  mnav_cancel is the exception (thread-safe, never takes the lock).  The owner destroys the
 * context under the lock and leaves ctx = nullptr: holders of the handle then refuse instead of touching freed memory. */
struct SharedContext {
  std::recursive_mutex mutex;                                         /* (recursive: makePlan's helpers lock on their own) */
  mnav_ctx* ctx = nullptr;                                            /* nullptr once the owner destroyed it */
  explicit SharedContext(mnav_ctx* c) : ctx(c) {}
  void destroy()
  {
    std::lock_guard<std::recursive_mutex> lock(mutex);
    if (ctx) mnav_destroy(ctx);
    ctx = nullptr;
  }
};
using ContextHandle = std::shared_ptr<SharedContext>;

/* Where the field of a map's last successful plan is resident. */
struct ResidentField { ContextHandle dev; uint32_t slot = 0, seed_face = MNAV_NONE; };

namespace detail {
inline std::mutex& field_mutex() { static std::mutex m; return m; }
inline std::map<const void*, ResidentField>& field_table() { static std::map<const void*, ResidentField> t; return t; }
}  // namespace detail

/* planner side: after a SUCCESSFUL plan on `map` (any pointer both plugins see, i.e. the MeshMap) */
inline void publish_field(const void* map, const ContextHandle& dev, uint32_t slot, uint32_t seed_face)
{
  std::lock_guard<std::mutex> lock(detail::field_mutex());
  detail::field_table()[map] = ResidentField{ dev, slot, seed_face };
}
/* controller side (setPlan) */
inline bool lookup_field(const void* map, ResidentField& out)
{
  std::lock_guard<std::mutex> lock(detail::field_mutex());
  const auto it = detail::field_table().find(map);
  if (it == detail::field_table().end()) return false;
  out = it->second;
  return true;
}

class FieldFollower {
public:
  mnav_follow_config config = MNAV_FOLLOW_CONFIG_DEFAULTS;            /* mesh_controller.h:192-201 */

  /* :179-193.  goal: position and orientation (x y z w) of the plan's last pose */
  bool setPlan(const double goal_position[3], const double goal_q_xyzw[4], const ResidentField& field)
  {
    if (!field.dev) return false;
    std::lock_guard<std::recursive_mutex> lock(field.dev->mutex);
    if (!field.dev->ctx) return false;                                /* the planner's context is gone */
    field_ = field;                                                   /* :182: the field stays where the planner left it */
    const double x_axis[3] = { 1.0, 0.0, 0.0 };
    for (int k = 0; k < 3; ++k) goal_pos_[k] = (float)goal_position[k];   /* :186 */
    direction_of(goal_q_xyzw, x_axis, goal_dir_);                     /* :187 */
    cancel_requested_ = false;                                        /* :190 */
    current_face_ = MNAV_NONE;                                        /* :191 */
    return true;
  }

  /* :67-170.  cmd: linear x, angular z (written on FOLLOW_SUCCESS / FOLLOW_CANCELED only) */
  uint32_t computeVelocityCommands(const double position[3], const double q_xyzw[4], double cmd[2], std::string& message)
  {
    if (!field_.dev) { message = "setPlan has not been called"; return FOLLOW_INTERNAL_ERROR; }
    std::lock_guard<std::recursive_mutex> lock(field_.dev->mutex);    /* waits for a plan that runs on this context */
    mnav_ctx* const ctx = field_.dev->ctx;
    if (!ctx) { message = "the planner that owned the field's device context is gone"; return FOLLOW_INTERNAL_ERROR; }
    const double x_axis[3] = { 1.0, 0.0, 0.0 }, z_axis[3] = { 0.0, 0.0, 1.0 };
    float up[3];
    for (int k = 0; k < 3; ++k) robot_pos_[k] = (float)position[k];  /* :74 */
    direction_of(q_xyzw, x_axis, robot_dir_);                         /* :75 */
    direction_of(q_xyzw, z_axis, up);                                 /* :159 */
    int32_t code = MNAV_FOLLOW_OUT_OF_MAP;
    uint32_t face = MNAV_NONE;
    float pos_out[3] = { robot_pos_[0], robot_pos_[1], robot_pos_[2] };
    double c[2] = { 0.0, 0.0 };
    /* :79-162 on the device, one robot */
    if (mnav_follow_batch(ctx, 1, robot_pos_, robot_dir_, up, &current_face_, &field_.slot, field_.seed_face == MNAV_NONE ? nullptr : &field_.seed_face,
                          &config, &code, &face, nullptr, pos_out, nullptr, nullptr, c, nullptr) != 0) {
      message = mnav_last_error(ctx);
      return FOLLOW_INTERNAL_ERROR;
    }
    if (code == MNAV_FOLLOW_OUT_OF_MAP) return FOLLOW_OUT_OF_MAP;     /* :96, :142 (current_face_ and robot_pos_ stay as they are) */
    current_face_ = face;                                             /* :86, :122, :134 */
    for (int k = 0; k < 3; ++k) robot_pos_[k] = pos_out[k];           /* :91, :125, :137 (kept when the face still held it) */
    if (code == MNAV_FOLLOW_NO_FIELD) { message = "Could not access vector field for the given face!"; return FOLLOW_FAILURE; }   /* :151-156 */
    cmd[0] = c[0];                                                    /* :161 */
    cmd[1] = c[1];                                                    /* :162 */
    if (cancel_requested_) return FOLLOW_CANCELED;                    /* :165-168 */
    return FOLLOW_SUCCESS;
  }

  /* :172-177, lvr2's float vector operations */
  bool isGoalReached(double dist_tolerance, double angle_tolerance) const
  {
    const float dx = goal_pos_[0] - robot_pos_[0], dy = goal_pos_[1] - robot_pos_[1], dz = goal_pos_[2] - robot_pos_[2];
    const float goal_distance = std::sqrt(dx * dx + dy * dy + dz * dz);                                                   /* :174 */
    const float angle = std::acos(goal_dir_[0] * robot_dir_[0] + goal_dir_[1] * robot_dir_[1] + goal_dir_[2] * robot_dir_[2]);   /* :175 */
    return goal_distance <= static_cast<float>(dist_tolerance) && angle <= static_cast<float>(angle_tolerance);          /* :176 */
  }

  bool cancel() { cancel_requested_ = true; return true; }           /* :195-200 */

  uint32_t currentFace() const { return current_face_; }
  const float* robotPosition() const { return robot_pos_; }

private:
  ResidentField field_;
  float goal_pos_[3] = { 0, 0, 0 }, goal_dir_[3] = { 1, 0, 0 }, robot_pos_[3] = { 0, 0, 0 }, robot_dir_[3] = { 1, 0, 0 };
  uint32_t current_face_ = MNAV_NONE;                                 /* lvr2::OptionalFaceHandle */
  std::atomic_bool cancel_requested_{ false };
};

}  // namespace mnav_host
