// gpu_mesh_controller.h -- mesh_controller::MeshController (mesh_controller/include/mesh_controller/mesh_controller.h:46-202)
// on top of mnav_follow_batch (include/mnav.h): the vector field the planners leave resident on the device is followed
// there, nothing V-sized comes to the host.  The reference copies MeshMap::getVectorMap in setPlan (:182) -- the
// setVectorMap side effect of the planners; here setPlan is told which device context and which plan of its last call
// hold the field instead.  The tick (current face, neighbour search, global search, directionAtPosition, cost,
// naiveControl, saturation) is ONE call with n = 1; what the reference keeps between ticks (current_face_, robot_pos_,
// robot_dir_, the goal) and the conversion of the pose's quaternion are mnav_host::FieldFollower
// (include/mnav_controller_host.hpp), shared with the ROS 2 plugin package; this file binds it to the ROS-free host types.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "../../../include/mnav.h"
#include "../../../include/mnav_controller_host.hpp"
#include "mesh_map_host.h"

namespace mesh_controller {

class MeshController {
public:
  // The outcomes computeVelocityCommands returns, named like the constants of mbf_msgs::action::ExePath::Result they
  // stand for.  The VALUES are this class's own (the message package is not part of this tree): the ROS plugin maps
  // them to the named constants.
  enum Outcome : uint32_t { SUCCESS = mnav_host::FOLLOW_SUCCESS, OUT_OF_MAP = mnav_host::FOLLOW_OUT_OF_MAP, FAILURE = mnav_host::FOLLOW_FAILURE,
                            CANCELED = mnav_host::FOLLOW_CANCELED, INTERNAL_ERROR = mnav_host::FOLLOW_INTERNAL_ERROR };
  struct Twist { double linear_x = 0.0, angular_z = 0.0; };           // cmd_vel.twist.linear.x / .angular.z (:161-162)

  bool initialize(const std::string& plugin_name, const std::shared_ptr<mesh_map::MeshMap>& mesh_map_ptr,
                  const rclcpp::Node::SharedPtr& node);                // :272-360
  // :179-193.  dev / slot: where the plan's vector map is resident (the planner's deviceContext(), the plan's index in its
  // last call); seed_face: the plan's seed face (CVP), MNAV_NONE otherwise.
  bool setPlan(const std::vector<geometry_msgs::msg::PoseStamped>& plan, const mnav_host::ContextHandle& dev, uint32_t slot = 0,
               uint32_t seed_face = MNAV_NONE);
  uint32_t computeVelocityCommands(const geometry_msgs::msg::PoseStamped& pose, Twist& cmd_vel, std::string& message);   // :67-170
  bool isGoalReached(double dist_tolerance, double angle_tolerance);  // :172-177
  bool cancel();                                                      // :195-200

  // poseToDirectionVector (:202-213): tf2's quaternion-to-basis product applied to `axis`, in double, narrowed to float
  static mesh_map::Normal poseToDirectionVector(const geometry_msgs::msg::PoseStamped& pose, const double axis[3]);
  static mesh_map::Vector poseToPositionVector(const geometry_msgs::msg::PoseStamped& pose);   // :215-218

  uint32_t currentFace() const { return follower_.currentFace(); }
  mesh_map::Vector robotPosition() const { const float* p = follower_.robotPosition(); return mesh_map::Vector(p[0], p[1], p[2]); }

private:
  std::shared_ptr<mesh_map::MeshMap> map_ptr_;
  rclcpp::Node::SharedPtr node_;
  std::string name_;
  mnav_host::FieldFollower follower_;
};

}  // namespace mesh_controller
