// adapter_capi.cpp -- tiny C harness around the C++ planner adapter so that the (Python) parity tests
// can drive makePlan()/cancel()/initialize() exactly like mbf_mesh_nav does
// (mbf_mesh_nav/src/mesh_navigation_server.cpp:185-212, mesh_planner_execution.cpp:55-66).
#include <cmath>
#include <cstring>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "gpu_mesh_controller.h"
#include "gpu_mesh_planners.h"
#include "mnav_planner_host.hpp"

struct mnav_adapter_planner {
  std::shared_ptr<mesh_map::MeshMap> map;
  rclcpp::Node::SharedPtr node;
  std::shared_ptr<mbf_mesh_core::MeshPlanner> planner;
  bool is_cvp = false;
  std::string message;
};

struct mnav_adapter_controller {
  mnav_host::ContextHandle dev;                             // the planner's device context (its handle outlives the planner)
  mesh_controller::MeshController controller;
};

extern "C" {

// kind: 0 = "dijkstra_mesh_planner/DijkstraMeshPlanner", 1 = "cvp_mesh_planner/CVPMeshPlanner"
mnav_adapter_planner* mnav_adapter_create(int kind, uint32_t V, uint32_t F, uint32_t E, const float* xyz, const uint32_t* faces,
                                          const uint32_t* edges, const float* vertex_normals, const float* face_normals,
                                          const float* vertex_costs, const float* edge_weights, const uint8_t* invalid,
                                          double goal_dist_offset, double cost_limit, double step_width)
{
  auto* a = new mnav_adapter_planner();
  a->map = std::make_shared<mesh_map::MeshMap>();
  mesh_map::MeshMap& m = *a->map;
  m.positions.assign(xyz, xyz + 3 * (size_t)V);
  m.faces.assign(faces, faces + 3 * (size_t)F);
  m.edges.assign(edges, edges + 2 * (size_t)E);
  m.vertex_normals.assign(vertex_normals, vertex_normals + 3 * (size_t)V);
  m.face_normals.assign(face_normals, face_normals + 3 * (size_t)F);
  m.vertex_costs.assign(vertex_costs, vertex_costs + V);
  m.edge_weights.assign(edge_weights, edge_weights + E);
  if (invalid) m.invalid.assign(invalid, invalid + V);
  m.finalize();
  a->node = std::make_shared<rclcpp::Node>();
  const std::string name = kind ? "cvp_mesh_planner" : "dijkstra_mesh_planner";
  a->node->set_override(name + ".goal_dist_offset", goal_dist_offset);
  a->node->set_override(name + ".cost_limit", cost_limit);
  a->node->set_override(name + ".step_width", step_width);
  a->is_cvp = kind != 0;
  if (kind) a->planner = std::make_shared<cvp_mesh_planner::CVPMeshPlanner>();
  else a->planner = std::make_shared<dijkstra_mesh_planner::DijkstraMeshPlanner>();
  if (!a->planner->initialize(name, a->map, a->node)) { delete a; return nullptr; }
  return a;
}

void mnav_adapter_destroy(mnav_adapter_planner* a) { delete a; }

// poses: x y z qx qy qz qw per pose.  Returns the MBF code; *n_poses = number of poses produced.
uint32_t mnav_adapter_make_plan(mnav_adapter_planner* a, const double start_pose[7], const double goal_pose[7], double* poses,
                                uint32_t cap, uint32_t* n_poses, double* cost, char* message, uint32_t message_cap)
{
  geometry_msgs::msg::PoseStamped s, g;
  auto fill = [](geometry_msgs::msg::PoseStamped& p, const double* v) {
    p.header.frame_id = "map";
    p.pose.position.x = v[0]; p.pose.position.y = v[1]; p.pose.position.z = v[2];
    p.pose.orientation.x = v[3]; p.pose.orientation.y = v[4]; p.pose.orientation.z = v[5]; p.pose.orientation.w = v[6];
  };
  fill(s, start_pose); fill(g, goal_pose);
  std::vector<geometry_msgs::msg::PoseStamped> plan;
  double c = 0;
  std::string msg;
  const uint32_t code = a->planner->makePlan(s, g, 0.0, plan, c, msg);
  *n_poses = (uint32_t)plan.size();
  for (uint32_t i = 0; i < plan.size() && i < cap; ++i) {
    const auto& p = plan[i].pose;
    double* o = poses + 7 * (size_t)i;
    o[0] = p.position.x; o[1] = p.position.y; o[2] = p.position.z;
    o[3] = p.orientation.x; o[4] = p.orientation.y; o[5] = p.orientation.z; o[6] = p.orientation.w;
  }
  *cost = c;
  if (message && message_cap) { std::strncpy(message, msg.c_str(), message_cap - 1); message[message_cap - 1] = 0; }
  return code;
}

// DijkstraMeshPlanner::makeFleetPlans after a makePlan: n start poses (7 doubles each) -> codes, pose counts and costs per
// robot; poses (7 doubles each, packed in robot order) when *total <= cap.  Returns the call's code, or 60 for a CVP planner.
uint32_t mnav_adapter_make_fleet_plans(mnav_adapter_planner* a, uint32_t n, const double* start_poses, uint32_t* codes, uint32_t* lens, double* costs,
                                       double* poses, uint64_t cap, uint64_t* total, char* message, uint32_t message_cap)
{
  if (a->is_cvp) return 60;
  std::vector<geometry_msgs::msg::PoseStamped> starts(n);
  for (uint32_t i = 0; i < n; ++i) {
    const double* v = start_poses + 7 * (size_t)i;
    auto& p = starts[i];
    p.header.frame_id = "map";
    p.pose.position.x = v[0]; p.pose.position.y = v[1]; p.pose.position.z = v[2];
    p.pose.orientation.x = v[3]; p.pose.orientation.y = v[4]; p.pose.orientation.z = v[5]; p.pose.orientation.w = v[6];
  }
  std::vector<std::vector<geometry_msgs::msg::PoseStamped>> plans;
  std::vector<double> c;
  std::vector<uint32_t> k;
  std::string msg;
  const uint32_t code = static_cast<dijkstra_mesh_planner::DijkstraMeshPlanner*>(a->planner.get())->makeFleetPlans(starts, plans, c, k, msg);
  uint64_t at = 0;
  for (uint32_t i = 0; i < n; ++i) {
    codes[i] = k[i]; lens[i] = (uint32_t)plans[i].size(); costs[i] = c[i];
    for (const auto& ps : plans[i]) {
      if (at < cap) {
        double* o = poses + 7 * (size_t)at;
        o[0] = ps.pose.position.x; o[1] = ps.pose.position.y; o[2] = ps.pose.position.z;
        o[3] = ps.pose.orientation.x; o[4] = ps.pose.orientation.y; o[5] = ps.pose.orientation.z; o[6] = ps.pose.orientation.w;
      }
      ++at;
    }
  }
  *total = at;
  if (message && message_cap) { std::strncpy(message, msg.c_str(), message_cap - 1); message[message_cap - 1] = 0; }
  return code;
}

int mnav_adapter_cancel(mnav_adapter_planner* a) { return a->planner->cancel() ? 1 : 0; }

// change counter of the map's cost arrays (0 = unknown: the device mirror hashes them on every plan)
void mnav_adapter_set_cost_version(mnav_adapter_planner* a, uint64_t version) { a->map->cost_version = version; }

// V-sized results of the last plan, fetched from the device on demand; what: 0 potential (float V), 1 predecessors
// (uint32 V; Dijkstra), 4 vector map (float V*3; Dijkstra)
int mnav_adapter_fetch(mnav_adapter_planner* a, int what, void* out)
{
  const uint32_t V = a->map->V;
  if (a->is_cvp) {
    auto* p = static_cast<cvp_mesh_planner::CVPMeshPlanner*>(a->planner.get());
    if (what != 0) return -1;
    std::memcpy(out, p->potential().data(), 4 * (size_t)V);
    return 0;
  }
  auto* p = static_cast<dijkstra_mesh_planner::DijkstraMeshPlanner*>(a->planner.get());
  if (what == 0) std::memcpy(out, p->potential().data(), 4 * (size_t)V);
  else if (what == 1) std::memcpy(out, p->predecessors().data(), 4 * (size_t)V);
  else if (what == 4) std::memcpy(out, p->getVectorMap().data(), 12 * (size_t)V);
  else return -1;
  return 0;
}

static void fill_layer_field(mesh_map::MeshMap::LayerVectorField& L, uint32_t V, const float* distances, const uint8_t* has_distance,
                             const float* vectors, const uint8_t* has_vector, double inscribed_radius, double inflation_radius,
                             double lethal_value, double inscribed_value, int repulsive_field)
{
  L.distances.assign(distances, distances + V); L.has_distance.assign(has_distance, has_distance + V);
  L.vectors.assign(vectors, vectors + 3 * (size_t)V); L.has_vector.assign(has_vector, has_vector + V);
  L.inscribed_radius = inscribed_radius; L.inflation_radius = inflation_radius; L.lethal_value = lethal_value;
  L.inscribed_value = inscribed_value; L.repulsive_field = repulsive_field != 0;
}

// a layer's repulsive vector field (InflationLayer distances_ / vector_map_) for MeshMap::meshAhead (mesh_map.cpp:1099-1102)
void mnav_adapter_add_layer_field(mnav_adapter_planner* a, const float* distances, const uint8_t* has_distance, const float* vectors,
                                  const uint8_t* has_vector, double inscribed_radius, double inflation_radius, double lethal_value,
                                  double inscribed_value, int repulsive_field)
{
  a->map->layer_fields.emplace_back();
  fill_layer_field(a->map->layer_fields.back(), a->map->V, distances, has_distance, vectors, has_vector, inscribed_radius, inflation_radius,
                   lethal_value, inscribed_value, repulsive_field);
}

// update the map's cost arrays in place (what a layer change does, mesh_map.cpp:454-493)
void mnav_adapter_set_costs(mnav_adapter_planner* a, const float* vertex_costs, const float* edge_weights)
{
  a->map->vertex_costs.assign(vertex_costs, vertex_costs + a->map->V);
  a->map->edge_weights.assign(edge_weights, edge_weights + a->map->E);
}

// Host-only geometry entry points (no device involved) so the CPU test-suite can check the adapter's
// MeshMap stand-in (nearest vertex, containing face, vector-field back-tracking) on its own.
uint32_t mnav_adapter_host_nearest_vertex(uint32_t V, uint32_t F, const float* xyz, const uint32_t* faces, const float p[3])
{
  mesh_map::MeshMap m;
  m.positions.assign(xyz, xyz + 3 * (size_t)V); m.faces.assign(faces, faces + 3 * (size_t)F);
  m.finalize();
  return m.getNearestVertexHandle(mesh_map::Vector(p[0], p[1], p[2]));
}

uint32_t mnav_adapter_host_containing_face(uint32_t V, uint32_t F, const float* xyz, const uint32_t* faces, const float p[3])
{
  mesh_map::MeshMap m;
  m.positions.assign(xyz, xyz + 3 * (size_t)V); m.faces.assign(faces, faces + 3 * (size_t)F);
  m.finalize();
  return m.getContainingFace(mesh_map::Vector(p[0], p[1], p[2]), 0.4f);
}

// The host pose loop (mnav_host::vertex_path_poses with mesh_map::calculatePoseFromPosition, what makePlan runs per plan) over
// the packed ids of mnav_fleet_paths for n robots on one thread: robot i's ids are ids[offsets[i] .. offsets[i + 1]), seed
// first; its poses (one more than its ids, none without ids) are packed in robot order.  No device involved: what a fleet
// caller does without mnav_fleet_plans, for tools/fleet_plans_perf.py.  Returns the pose count.
uint64_t mnav_adapter_host_vertex_path_poses(const float* xyz, const float* vertex_normals, uint32_t n, const uint32_t* ids, const uint64_t* offsets,
                                             const uint32_t* slots, const float* start_pos, const float* goal_pos, double* poses, double* costs)
{
  uint64_t at = 0;
  std::vector<uint32_t> path;
  std::vector<geometry_msgs::msg::PoseStamped> plan;
  const geometry_msgs::msg::PoseStamped stamped;
  auto vec = [](const float* p, size_t i) { return mesh_map::Vector(p[3 * i], p[3 * i + 1], p[3 * i + 2]); };
  for (uint32_t i = 0; i < n; ++i) {
    path.assign(std::make_reverse_iterator(ids + offsets[i + 1]), std::make_reverse_iterator(ids + offsets[i]));   // robot side first (:83)
    plan.clear();
    mnav_host::vertex_path_poses(path, vec(start_pos, i), vec(goal_pos, slots[i]), stamped, [&](uint32_t v) { return vec(xyz, v); },
                                 [&](uint32_t v) { return vec(vertex_normals, v); },
                                 [](const mesh_map::Vector& from, const mesh_map::Vector& to, const mesh_map::Normal& up, float& len) {
                                   return mesh_map::calculatePoseFromPosition(from, to, up, len);
                                 },
                                 plan, costs[i]);
    for (const auto& ps : plan) {
      double* o = poses + 7 * (size_t)at++;
      o[0] = ps.pose.position.x; o[1] = ps.pose.position.y; o[2] = ps.pose.position.z;
      o[3] = ps.pose.orientation.x; o[4] = ps.pose.orientation.y; o[5] = ps.pose.orientation.z; o[6] = ps.pose.orientation.w;
    }
  }
  return at;
}

// The same for the packed rows of mnav_fleet_walks (mnav_host::face_path_poses): one pose per entry, the goal pose last.
uint64_t mnav_adapter_host_face_path_poses(const float* face_normals, uint32_t n, const float* positions, const uint32_t* faces, const uint64_t* offsets,
                                           const uint32_t* slots, const double* goal_pose, double* poses, double* costs)
{
  uint64_t at = 0;
  std::vector<std::pair<mesh_map::Vector, uint32_t>> path;
  std::vector<geometry_msgs::msg::PoseStamped> plan;
  const geometry_msgs::msg::PoseStamped stamped;
  for (uint32_t i = 0; i < n; ++i) {
    path.clear();
    for (uint64_t q = offsets[i + 1]; q-- > offsets[i];) path.push_back({ mesh_map::Vector(positions[3 * q], positions[3 * q + 1], positions[3 * q + 2]), faces[q] });   // robot side first (:93)
    const double* g = goal_pose + 7 * (size_t)slots[i];
    geometry_msgs::msg::Pose goal;
    goal.position.x = g[0]; goal.position.y = g[1]; goal.position.z = g[2];
    goal.orientation.x = g[3]; goal.orientation.y = g[4]; goal.orientation.z = g[5]; goal.orientation.w = g[6];
    plan.clear();
    mnav_host::face_path_poses(path, false, goal, stamped,
                               [&](uint32_t f) { return mesh_map::Normal(face_normals[3 * (size_t)f], face_normals[3 * (size_t)f + 1], face_normals[3 * (size_t)f + 2]); },
                               [](const mesh_map::Vector& from, const mesh_map::Vector& to, const mesh_map::Normal& up, float& len) {
                                 return mesh_map::calculatePoseFromPosition(from, to, up, len);
                               },
                               plan, costs[i]);
    for (const auto& ps : plan) {
      double* o = poses + 7 * (size_t)at++;
      o[0] = ps.pose.position.x; o[1] = ps.pose.position.y; o[2] = ps.pose.position.z;
      o[3] = ps.pose.orientation.x; o[4] = ps.pose.orientation.y; o[5] = ps.pose.orientation.z; o[6] = ps.pose.orientation.w;
    }
  }
  return at;
}

// cvp_mesh_planner.cpp:920-951 on a given vector field; path in reference list order (seed first)
static uint32_t host_backtrack(mesh_map::MeshMap& m, uint32_t V, const float* vecmap, const uint8_t* has_vec, const float seed_pos[3],
                               uint32_t seed_face, const float target_pos[3], uint32_t target_face, double step_width, uint32_t cap,
                               float* path_pos, uint32_t* path_face, uint32_t* path_len);

// the same with one layer vector field (Inflation) added in meshAhead; code 54 + *panicked = 1 where the reference's
// attribute-map lookup panics
uint32_t mnav_adapter_host_backtrack_layer(uint32_t V, uint32_t F, const float* xyz, const uint32_t* faces, const float* vecmap,
                                           const uint8_t* has_vec, const float seed_pos[3], uint32_t seed_face, const float target_pos[3],
                                           uint32_t target_face, double step_width, const float* distances, const uint8_t* has_distance,
                                           const float* vectors, const uint8_t* has_vector, double inscribed_radius, double inflation_radius,
                                           double lethal_value, double inscribed_value, int repulsive_field, uint32_t cap, float* path_pos,
                                           uint32_t* path_face, uint32_t* path_len, int* panicked)
{
  mesh_map::MeshMap m;
  m.positions.assign(xyz, xyz + 3 * (size_t)V); m.faces.assign(faces, faces + 3 * (size_t)F);
  m.finalize();
  m.layer_fields.emplace_back();
  fill_layer_field(m.layer_fields.back(), V, distances, has_distance, vectors, has_vector, inscribed_radius, inflation_radius, lethal_value,
                   inscribed_value, repulsive_field);
  *panicked = 0;
  try {
    return host_backtrack(m, V, vecmap, has_vec, seed_pos, seed_face, target_pos, target_face, step_width, cap, path_pos, path_face, path_len);
  } catch (const mesh_map::MeshMap::MapPanic&) { *panicked = 1; *path_len = 0; return 54; }
}

uint32_t mnav_adapter_host_backtrack(uint32_t V, uint32_t F, const float* xyz, const uint32_t* faces, const float* vecmap,
                                     const uint8_t* has_vec, const float seed_pos[3], uint32_t seed_face, const float target_pos[3],
                                     uint32_t target_face, double step_width, uint32_t cap, float* path_pos, uint32_t* path_face,
                                     uint32_t* path_len)
{
  mesh_map::MeshMap m;
  m.positions.assign(xyz, xyz + 3 * (size_t)V); m.faces.assign(faces, faces + 3 * (size_t)F);
  m.finalize();
  return host_backtrack(m, V, vecmap, has_vec, seed_pos, seed_face, target_pos, target_face, step_width, cap, path_pos, path_face, path_len);
}

static uint32_t host_backtrack(mesh_map::MeshMap& m, uint32_t V, const float* vecmap, const uint8_t* has_vec, const float seed_pos[3],
                               uint32_t seed_face, const float target_pos[3], uint32_t target_face, double step_width, uint32_t cap,
                               float* path_pos, uint32_t* path_face, uint32_t* path_len)
{
  m.setVectorMap(std::vector<float>(vecmap, vecmap + 3 * (size_t)V), std::vector<uint8_t>(has_vec, has_vec + V));
  const mesh_map::Vector start(seed_pos[0], seed_pos[1], seed_pos[2]);
  mesh_map::Vector pos(target_pos[0], target_pos[1], target_pos[2]);
  uint32_t face = target_face;
  std::vector<std::pair<mesh_map::Vector, uint32_t>> rev;
  rev.push_back({ pos, face });
  uint32_t code = 0;
  while (pos.distance2(start) > step_width) {
    if (m.meshAhead(pos, face, (float)step_width)) rev.push_back({ pos, face });
    else { code = 54; break; }
    if (rev.size() >= cap) { code = 54; break; }
  }
  if (code == 0) rev.push_back({ start, seed_face });
  uint32_t n = 0;
  for (size_t i = rev.size(); i-- > 0 && n < cap; ++n) {
    path_pos[3 * n] = rev[i].first.x; path_pos[3 * n + 1] = rev[i].first.y; path_pos[3 * n + 2] = rev[i].first.z;
    path_face[n] = rev[i].second;
  }
  *path_len = n;
  return code;
}

// -- mesh_controller::MeshController over the planner's map and device context, driven like mbf_mesh_nav drives a
// controller plugin (mesh_controller_execution.cpp): setPlan, computeVelocityCommands per tick, isGoalReached, cancel.
// cfg: the eight parameters of mesh_controller.h:193-200 in that order, or null for the defaults.
mnav_adapter_controller* mnav_adapter_controller_create(mnav_adapter_planner* a, const double* cfg)
{
  static const char* names[8] = { "max_lin_velocity", "max_ang_velocity", "arrival_fading", "ang_vel_factor", "lin_vel_factor", "max_angle",
                                  "max_search_radius", "max_search_distance" };
  if (!a) return nullptr;
  auto* c = new mnav_adapter_controller();
  c->dev = a->is_cvp ? static_cast<cvp_mesh_planner::CVPMeshPlanner*>(a->planner.get())->deviceContext()
                     : static_cast<dijkstra_mesh_planner::DijkstraMeshPlanner*>(a->planner.get())->deviceContext();
  auto node = std::make_shared<rclcpp::Node>();
  if (cfg) for (int k = 0; k < 8; ++k) node->set_override(std::string("mesh_controller.") + names[k], cfg[k]);
  if (!c->controller.initialize("mesh_controller", a->map, node)) { delete c; return nullptr; }
  return c;
}

void mnav_adapter_controller_destroy(mnav_adapter_controller* c) { delete c; }

// poses: x y z qx qy qz qw per pose (the plan makePlan produced); slot: the plan's index in the planner's last call;
// seed_face: the plan's seed face or 0xFFFFFFFF
int mnav_adapter_controller_set_plan(mnav_adapter_controller* c, const double* poses, uint32_t n, uint32_t slot, uint32_t seed_face)
{
  std::vector<geometry_msgs::msg::PoseStamped> plan(n);
  for (uint32_t i = 0; i < n; ++i) {
    const double* v = poses + 7 * (size_t)i;
    auto& p = plan[i].pose;
    p.position.x = v[0]; p.position.y = v[1]; p.position.z = v[2];
    p.orientation.x = v[3]; p.orientation.y = v[4]; p.orientation.z = v[5]; p.orientation.w = v[6];
  }
  return c->controller.setPlan(plan, c->dev, slot, seed_face) ? 1 : 0;
}

// one tick.  Returns the controller's Outcome (0 SUCCESS, 1 OUT_OF_MAP, 2 FAILURE, 3 CANCELED, 4 INTERNAL_ERROR);
// cmd = linear x, angular z; face / pos = what the controller keeps for the next tick
uint32_t mnav_adapter_controller_compute(mnav_adapter_controller* c, const double pose[7], double cmd[2], uint32_t* face, float pos[3], char* message,
                                         uint32_t message_cap)
{
  geometry_msgs::msg::PoseStamped p;
  p.pose.position.x = pose[0]; p.pose.position.y = pose[1]; p.pose.position.z = pose[2];
  p.pose.orientation.x = pose[3]; p.pose.orientation.y = pose[4]; p.pose.orientation.z = pose[5]; p.pose.orientation.w = pose[6];
  mesh_controller::MeshController::Twist t;
  std::string msg;
  const uint32_t code = c->controller.computeVelocityCommands(p, t, msg);
  cmd[0] = t.linear_x; cmd[1] = t.angular_z;
  *face = c->controller.currentFace();
  const mesh_map::Vector r = c->controller.robotPosition();
  pos[0] = r.x; pos[1] = r.y; pos[2] = r.z;
  if (message && message_cap) { std::strncpy(message, msg.c_str(), message_cap - 1); message[message_cap - 1] = 0; }
  return code;
}

int mnav_adapter_controller_goal_reached(mnav_adapter_controller* c, double dist_tolerance, double angle_tolerance)
{
  return c->controller.isGoalReached(dist_tolerance, angle_tolerance) ? 1 : 0;
}

int mnav_adapter_controller_cancel(mnav_adapter_controller* c) { return c->controller.cancel() ? 1 : 0; }

// heading (axis 0: x) or up vector (axis 2: z) of a pose, as the controller derives it from the quaternion
void mnav_adapter_controller_direction(const double pose[7], int axis, float out[3])
{
  geometry_msgs::msg::PoseStamped p;
  p.pose.orientation.x = pose[3]; p.pose.orientation.y = pose[4]; p.pose.orientation.z = pose[5]; p.pose.orientation.w = pose[6];
  const double a[3] = { axis == 0 ? 1.0 : 0.0, axis == 1 ? 1.0 : 0.0, axis == 2 ? 1.0 : 0.0 };
  const mesh_map::Normal v = mesh_controller::MeshController::poseToDirectionVector(p, a);
  out[0] = v.x; out[1] = v.y; out[2] = v.z;
}

// What the reference's controller reads: MeshMap::directionAtPosition (mesh_map.cpp:625-650) over the vector map the
// planner's setVectorMap left in the HOST map.  1 + out = the direction, 0 = none (no field on the host).
int mnav_adapter_host_direction(mnav_adapter_planner* a, uint32_t face, const float bary[3], float out[3])
{
  const mesh_map::MeshMap& m = *a->map;
  if (face >= m.F || m.vector_map_set.size() != m.V) return 0;
  const uint32_t* vs = &m.faces[3 * (size_t)face];
  if (!(m.vector_map_set[vs[0]] || m.vector_map_set[vs[1]] || m.vector_map_set[vs[2]])) return 0;   // :633
  mesh_map::Vector vec(0, 0, 0);
  for (int k = 0; k < 3; ++k)
    if (m.vector_map_set[vs[k]]) vec = vec + mesh_map::Vector(m.vector_map[3 * (size_t)vs[k]], m.vector_map[3 * (size_t)vs[k] + 1], m.vector_map[3 * (size_t)vs[k] + 2]) * bary[k];   // :636-638
  if (!(std::isfinite(vec.x) && std::isfinite(vec.y) && std::isfinite(vec.z))) return 0;           // :639
  out[0] = vec.x; out[1] = vec.y; out[2] = vec.z;
  return 1;
}

}  // extern "C"
