// mesh_gpu_planners/GpuMeshController -- the vector-field follower as a REAL mbf_mesh_core::MeshController plugin.
//
//   mesh_gpu_planners/GpuMeshController  takes the place of  mesh_controller/MeshController  beside the GPU planners
//
// Same ROS parameters (<name>.max_lin_velocity 1.0, .max_ang_velocity 0.5, .arrival_fading 0.5, .ang_vel_factor 1.0,
// .lin_vel_factor 1.0, .max_angle 20, .max_search_radius 0.4, .max_search_distance 0.4), same result codes.  The reference
// copies the field out of the map in setPlan (mesh_controller.cpp:182), which is why its planners call
// MeshMap::setVectorMap; this controller follows the field where the GPU planners of this package leave it -- resident on
// the device -- so they can run with `sync_vector_map` off and nothing V-sized crosses PCIe per plan or per tick.  The
// planner publishes (context handle, plan, seed face) under the MeshMap pointer after every successful plan
// (mnav_host::publish_field), setPlan looks it up.  Planner and controller run on different threads of Move Base Flex:
// both take the lock of the shared context handle around their device calls, and the handle outlives the planner
// (mnav_host::SharedContext).  A tick follows the field of the planner's LAST plan, not a copy taken in setPlan: what
// that means for a replan is in INTEGRATION.md.
//
// The logic is mnav_host::FieldFollower (include/mnav_controller_host.hpp), shared with and tested through the ROS-free
// adapter (mesh_navigation_amd/csrc/adapter/gpu_mesh_controller.h); this class only converts message types and maps the
// outcomes to the named constants of mbf_msgs::action::ExePath::Result.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include <mbf_mesh_core/mesh_controller.h>
#include <mbf_msgs/action/exe_path.hpp>
#include <mesh_map/mesh_map.h>
#include <rclcpp/rclcpp.hpp>

#include "mnav.h"
#include "mnav_controller_host.hpp"

namespace mesh_gpu_planners
{
class GpuMeshController : public mbf_mesh_core::MeshController
{
public:
  typedef std::shared_ptr<GpuMeshController> Ptr;
  GpuMeshController() = default;
  ~GpuMeshController() override = default;
  uint32_t computeVelocityCommands(const geometry_msgs::msg::PoseStamped& pose, const geometry_msgs::msg::TwistStamped& velocity,
                                   geometry_msgs::msg::TwistStamped& cmd_vel, std::string& message) override;   // mesh_controller.cpp:67-170
  bool isGoalReached(double dist_tolerance, double angle_tolerance) override;                                   // :172-177
  bool setPlan(const std::vector<geometry_msgs::msg::PoseStamped>& plan) override;                              // :179-193
  bool cancel() override;                                                                                       // :195-200
  bool initialize(const std::string& plugin_name, const std::shared_ptr<tf2_ros::Buffer>& tf_ptr,
                  const std::shared_ptr<mesh_map::MeshMap>& mesh_map_ptr, const rclcpp::Node::SharedPtr& node) override;   // :272-360
private:
  rcl_interfaces::msg::SetParametersResult reconfigureCallback(std::vector<rclcpp::Parameter> parameters);     // :244-270
  rclcpp::Node::SharedPtr node_;
  std::string name_;
  std::shared_ptr<mesh_map::MeshMap> map_ptr_;
  rclcpp::node_interfaces::OnSetParametersCallbackHandle::SharedPtr reconfiguration_callback_handle_;
  mnav_host::FieldFollower follower_;
};
}  // namespace mesh_gpu_planners
