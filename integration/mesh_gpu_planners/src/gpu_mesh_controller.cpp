// gpu_mesh_controller.cpp -- see gpu_mesh_controller.h.  Reference line numbers (mesh_controller.cpp) in the comments.
#include "mesh_gpu_planners/gpu_mesh_controller.h"

#include <functional>

#include <pluginlib/class_list_macros.hpp>

PLUGINLIB_EXPORT_CLASS(mesh_gpu_planners::GpuMeshController, mbf_mesh_core::MeshController);

using geometry_msgs::msg::PoseStamped;
typedef mbf_msgs::action::ExePath::Result Result;

namespace mesh_gpu_planners
{
static void split(const PoseStamped& pose, double position[3], double q_xyzw[4])
{
  position[0] = pose.pose.position.x; position[1] = pose.pose.position.y; position[2] = pose.pose.position.z;
  q_xyzw[0] = pose.pose.orientation.x; q_xyzw[1] = pose.pose.orientation.y; q_xyzw[2] = pose.pose.orientation.z; q_xyzw[3] = pose.pose.orientation.w;
}

uint32_t GpuMeshController::computeVelocityCommands(const PoseStamped& pose, const geometry_msgs::msg::TwistStamped& /*velocity*/,
                                                    geometry_msgs::msg::TwistStamped& cmd_vel, std::string& message)
{
  double position[3], q[4], cmd[2] = { 0.0, 0.0 };
  split(pose, position, q);
  const uint32_t outcome = follower_.computeVelocityCommands(position, q, cmd, message);
  switch (outcome) {
    case mnav_host::FOLLOW_OUT_OF_MAP: return Result::OUT_OF_MAP;                                  // :96, :142
    case mnav_host::FOLLOW_FAILURE:
      RCLCPP_ERROR_STREAM(node_->get_logger(), "Could not access vector field for the given face!");   // :154
      return Result::FAILURE;                                                                      // :155
    case mnav_host::FOLLOW_INTERNAL_ERROR:
      RCLCPP_ERROR_STREAM(node_->get_logger(), name_ << ": " << message);
      return Result::INTERNAL_ERROR;
    default: break;
  }
  cmd_vel.twist.linear.x = cmd[0];                                                                 // :161
  cmd_vel.twist.angular.z = cmd[1];                                                                // :162
  cmd_vel.header.stamp = node_->now();                                                             // :163
  return outcome == mnav_host::FOLLOW_CANCELED ? Result::CANCELED : Result::SUCCESS;              // :165-169
}

bool GpuMeshController::isGoalReached(double dist_tolerance, double angle_tolerance)
{
  return follower_.isGoalReached(dist_tolerance, angle_tolerance);
}

bool GpuMeshController::setPlan(const std::vector<PoseStamped>& plan)
{
  if (plan.empty()) return false;
  mnav_host::ResidentField field;
  if (!mnav_host::lookup_field(map_ptr_.get(), field)) {
    RCLCPP_ERROR_STREAM(node_->get_logger(), name_ << ": no GPU planner of this process has planned on this map yet: there is no resident field to follow");
    return false;
  }
  double position[3], q[4];
  split(plan.back(), position, q);                                                                 // :186-187
  return follower_.setPlan(position, q, field);
}

bool GpuMeshController::cancel()
{
  RCLCPP_INFO_STREAM(node_->get_logger(), "The MeshController has been requested to cancel!");    // :197
  return follower_.cancel();
}

rcl_interfaces::msg::SetParametersResult GpuMeshController::reconfigureCallback(std::vector<rclcpp::Parameter> parameters)
{
  rcl_interfaces::msg::SetParametersResult result;
  mnav_follow_config& c = follower_.config;
  for (const auto& parameter : parameters) {                                                       // :248-266
    const std::string& n = parameter.get_name();
    if (n == name_ + ".max_lin_velocity") c.max_lin_velocity = parameter.as_double();
    else if (n == name_ + ".max_ang_velocity") c.max_ang_velocity = parameter.as_double();
    else if (n == name_ + ".arrival_fading") c.arrival_fading = parameter.as_double();
    else if (n == name_ + ".ang_vel_factor") c.ang_vel_factor = parameter.as_double();
    else if (n == name_ + ".lin_vel_factor") c.lin_vel_factor = parameter.as_double();
    else if (n == name_ + ".max_angle") c.max_angle = parameter.as_double();
    else if (n == name_ + ".max_search_radius") c.max_search_radius = parameter.as_double();
    else if (n == name_ + ".max_search_distance") c.max_search_distance = parameter.as_double();
  }
  result.successful = true;
  return result;
}

bool GpuMeshController::initialize(const std::string& plugin_name, const std::shared_ptr<tf2_ros::Buffer>& /*tf_ptr*/,
                                   const std::shared_ptr<mesh_map::MeshMap>& mesh_map_ptr, const rclcpp::Node::SharedPtr& node)
{
  node_ = node;                                                                                    // :277
  map_ptr_ = mesh_map_ptr;                                                                         // :278
  name_ = plugin_name;                                                                             // :279
  mnav_follow_config& c = follower_.config;
  c.max_lin_velocity = node_->declare_parameter(name_ + ".max_lin_velocity", c.max_lin_velocity);             // :290
  c.max_ang_velocity = node_->declare_parameter(name_ + ".max_ang_velocity", c.max_ang_velocity);             // :299
  c.arrival_fading = node_->declare_parameter(name_ + ".arrival_fading", c.arrival_fading);                   // :308
  c.ang_vel_factor = node_->declare_parameter(name_ + ".ang_vel_factor", c.ang_vel_factor);                   // :317
  c.lin_vel_factor = node_->declare_parameter(name_ + ".lin_vel_factor", c.lin_vel_factor);                   // :326
  c.max_angle = node_->declare_parameter(name_ + ".max_angle", c.max_angle);                                  // :335
  c.max_search_radius = node_->declare_parameter(name_ + ".max_search_radius", c.max_search_radius);          // :344
  c.max_search_distance = node_->declare_parameter(name_ + ".max_search_distance", c.max_search_distance);    // :353
  reconfiguration_callback_handle_ = node_->add_on_set_parameters_callback(                                    // :356-357
      std::bind(&GpuMeshController::reconfigureCallback, this, std::placeholders::_1));
  return true;
}
}  // namespace mesh_gpu_planners
