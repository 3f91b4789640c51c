// gpu_mesh_controller.cpp -- see gpu_mesh_controller.h.  Reference line numbers (mesh_controller.cpp) in the comments.
#include "gpu_mesh_controller.h"

using geometry_msgs::msg::PoseStamped;

namespace mesh_controller {

static void split(const PoseStamped& pose, double position[3], double q_xyzw[4])
{
  position[0] = pose.pose.position.x; position[1] = pose.pose.position.y; position[2] = pose.pose.position.z;
  q_xyzw[0] = pose.pose.orientation.x; q_xyzw[1] = pose.pose.orientation.y; q_xyzw[2] = pose.pose.orientation.z; q_xyzw[3] = pose.pose.orientation.w;
}

bool MeshController::initialize(const std::string& plugin_name, const std::shared_ptr<mesh_map::MeshMap>& mesh_map_ptr,
                                const rclcpp::Node::SharedPtr& node)
{
  node_ = node;                                                       // :277
  map_ptr_ = mesh_map_ptr;                                            // :278
  name_ = plugin_name;                                                // :279
  if (node_) {
    mnav_follow_config& c = follower_.config;
    c.max_lin_velocity = node_->declare_parameter(name_ + ".max_lin_velocity", c.max_lin_velocity);             // :290
    c.max_ang_velocity = node_->declare_parameter(name_ + ".max_ang_velocity", c.max_ang_velocity);             // :299
    c.arrival_fading = node_->declare_parameter(name_ + ".arrival_fading", c.arrival_fading);                   // :308
    c.ang_vel_factor = node_->declare_parameter(name_ + ".ang_vel_factor", c.ang_vel_factor);                   // :317
    c.lin_vel_factor = node_->declare_parameter(name_ + ".lin_vel_factor", c.lin_vel_factor);                   // :326
    c.max_angle = node_->declare_parameter(name_ + ".max_angle", c.max_angle);                                  // :335
    c.max_search_radius = node_->declare_parameter(name_ + ".max_search_radius", c.max_search_radius);          // :344
    c.max_search_distance = node_->declare_parameter(name_ + ".max_search_distance", c.max_search_distance);    // :353
  }
  return map_ptr_ != nullptr;
}

bool MeshController::setPlan(const std::vector<PoseStamped>& plan, const mnav_host::ContextHandle& dev, uint32_t slot, uint32_t seed_face)
{
  if (plan.empty()) return false;
  double position[3], q[4];
  split(plan.back(), position, q);                                    // :186-187
  mnav_host::ResidentField field;
  field.dev = dev; field.slot = slot; field.seed_face = seed_face;
  return follower_.setPlan(position, q, field);
}

uint32_t MeshController::computeVelocityCommands(const PoseStamped& pose, Twist& cmd_vel, std::string& message)
{
  double position[3], q[4], cmd[2] = { cmd_vel.linear_x, cmd_vel.angular_z };
  split(pose, position, q);
  const uint32_t outcome = follower_.computeVelocityCommands(position, q, cmd, message);
  cmd_vel.linear_x = cmd[0];                                          // :161
  cmd_vel.angular_z = cmd[1];                                         // :162
  return outcome;
}

bool MeshController::isGoalReached(double dist_tolerance, double angle_tolerance) { return follower_.isGoalReached(dist_tolerance, angle_tolerance); }

bool MeshController::cancel() { return follower_.cancel(); }

mesh_map::Normal MeshController::poseToDirectionVector(const PoseStamped& pose, const double axis[3])
{
  double position[3], q[4];
  float v[3];
  split(pose, position, q);
  mnav_host::direction_of(q, axis, v);                                // :204-212
  return mesh_map::Normal(v[0], v[1], v[2]);
}

mesh_map::Vector MeshController::poseToPositionVector(const PoseStamped& pose)
{
  return mesh_map::Vector((float)pose.pose.position.x, (float)pose.pose.position.y, (float)pose.pose.position.z);   // :217
}

}  // namespace mesh_controller
