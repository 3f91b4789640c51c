// mnav_plans.h -- fleet plans (mnav_fleet_plans, mnav_fleet_walk_plans): MeshPlanner::makePlan's pose list and cost for
// many robots per resident field.
// Dijkstra (dijkstra_mesh_planner.cpp:83-116): a served robot with the hops u_0 = pred[v] ... u_{L-1} = seed (the reverse
// of the ids of mnav_fleet_paths) gets L + 1 poses
//   pose 0        pose_from(start_pos, xyz[u_0],     vn[u_0])
//   pose k        pose_from(xyz[u_{k-1}], xyz[u_k],  vn[u_{k-1}])      1 <= k < L
//   pose L        pose_from(xyz[u_{L-1}], goal_pos,  vn[u_{L-1}])
// and cost = the double sum of the L + 1 float lengths in that order; L == 0: no poses, cost 0.
// CVP (cvp_mesh_planner.cpp:93-124): a walk row of m entries in walk order (robot first, as k_backtrack leaves it)
// r_0 .. r_{m-1} gets m poses: pose q = pose_from(r_q.pos, r_{q+1}.pos, fn[r_q.face]) for q < m - 1, the goal pose
// verbatim at q = m - 1, cost = the ordered double sum of the m - 1 lengths.
// plan_pose / walk_pose / the cost loops are the device's own source and the host mirror's (tests/test_plans_model.py).
//
// Device shape: k_fleet_cut, k_fleet_len, the rule-5 passes and the 64-bit scan of mnav_fleet.h as they are; k_plan_count
// (one lane per robot: hops -> poses, block sums) in front of the scan, k_fleet_write into an id scratch that never leaves
// the device (robot i's hops at its pose offset: one spare word per robot), k_plan_poses (ONE LANE PER PACKED POSE: the
// robot by binary search over the offsets, three gathers, the pose, 56 B + the float length stored -- consecutive lanes,
// consecutive poses: a wave's stores form one dense run), k_plan_cost (one lane per robot: its lengths in order, in
// double).  The walks: k_backtrack's scratch rows are already robot first; k_walk_poses (one wave per robot, lane q = pose
// q) and k_walk_cost (one lane per robot over its row) read them chunk by chunk.
#pragma once
#include "mnav_fleet.h"
#include "mnav_pose.h"

namespace mnav_fleet {

using mnav::W3;

constexpr int kPoseDoubles = 7;    // x y z qx qy qz qw

MNAV_HD uint32_t plan_pose_count(uint32_t hops) { return hops ? hops + 1u : 0u; }

MNAV_HD W3 plan_load3(GPtr<const float> p, size_t i) { return mnav::w3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }

// What one packed pose reads.  off (n + 1): the exclusive scan of count; robot i's hops lie at ids[off[i] .. off[i] + count[i] - 1),
// seed first (fleet_write).
struct PlanView {
  uint32_t n, V;
  GPtr<const float> xyz, vn, start, goal;          // V x 3, V x 3, n x 3 (robot positions), plans x 3
  GPtr<const uint32_t> slot, count, ids;
  GPtr<const unsigned long long> off;
};

// the robot that owns packed pose g < off[n]: off[i] <= g < off[i + 1].  Robots without poses make equal neighbouring
// offsets; the search keeps off[lo] <= g < off[hi], so it ends on the last of them -- the one that has poses.
MNAV_HD uint32_t plan_robot_of(GPtr<const unsigned long long> off, uint32_t n, unsigned long long g)
{
  uint32_t lo = 0u, hi = n;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// the two ends and the normal of packed pose g
MNAV_HD void plan_pose_ends(const PlanView& Q, unsigned long long g, W3* current, W3* next, W3* normal)
{
  const uint32_t i = plan_robot_of(Q.off, Q.n, g);
  const unsigned long long o = Q.off[i];
  const uint32_t k = (uint32_t)(g - o), L = Q.count[i] - 1u;          // pose k of L + 1; hop u_q = ids[o + L - 1 - q]
  uint32_t a = Q.ids[o + (L - 1u - (k ? k - 1u : 0u))];               // the vertex whose normal is up: u_0 for pose 0, else u_{k-1}
  if (a >= Q.V) a = 0u;                                               // (never: fleet_classify has walked the chain)
  *normal = plan_load3(Q.vn, a);
  *current = k ? plan_load3(Q.xyz, a) : plan_load3(Q.start, i);
  if (k == L) *next = plan_load3(Q.goal, Q.slot[i]);
  else {
    uint32_t b = Q.ids[o + (L - 1u - k)];
    if (b >= Q.V) b = 0u;
    *next = plan_load3(Q.xyz, b);
  }
}

// pose: 7 doubles, or null: the length alone
MNAV_HD float plan_pose(const PlanView& Q, unsigned long long g, double* pose, int* branch_out = nullptr)
{
  W3 current, next, normal;
  plan_pose_ends(Q, g, &current, &next, &normal);
  if (!pose) return mnav::pose_step_length(current, next);
  return mnav::pose_from_position(current, next, normal, pose, branch_out);
}

// one robot's lengths in order, in double (:89, :107, :114)
MNAV_HD double plan_cost(GPtr<const float> lengths, unsigned long long o, uint32_t count)
{
  double cost = 0.0;
  for (uint32_t k = 0; k < count; ++k) cost += lengths[o + k];
  return cost;
}

// A walk row in walk order (robot first): m entries of 3 floats and one face id.
struct WalkRow { GPtr<const float> pos; GPtr<const uint32_t> face; uint32_t m; };

// pose q of the row's m: the last one is the goal pose, bit for bit
MNAV_HD void walk_pose(const WalkRow& R, uint32_t q, GPtr<const float> face_normals, uint32_t F, GPtr<const double> goal_pose, double pose[kPoseDoubles])
{
  if (q + 1u >= R.m) {
    for (int c = 0; c < kPoseDoubles; ++c) pose[c] = goal_pose[c];    // :119-123
    return;
  }
  uint32_t f = R.face[q];
  if (f >= F) f = 0u;                                                 // (never: the walk only enters faces of the mesh)
  (void)mnav::pose_from_position(plan_load3(R.pos, q), plan_load3(R.pos, (size_t)q + 1u), plan_load3(face_normals, f), pose);   // :112
}

MNAV_HD double walk_cost(const WalkRow& R)
{
  double cost = 0.0;                                                  // :99
  for (uint32_t q = 0; q + 1u < R.m; ++q) cost += mnav::pose_step_length(plan_load3(R.pos, q), plan_load3(R.pos, (size_t)q + 1u));   // :113
  return cost;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// mnav_fleet_plans on host arrays, pass by pass as the device runs it.  count / off / cost per robot; poses: null, or
// 7 * off[n] doubles; branches[4] (optional): how often each branch of the quaternion was taken.
inline void fleet_plans_host(uint32_t n, uint32_t V, const Field* fields, const uint32_t* slot, const uint32_t* vtx, const float* xyz, const float* vn,
                             const float* start, const float* goal, uint32_t* code, uint32_t* count, float* potential, unsigned long long* off, double* cost,
                             double* poses, uint32_t* counters, uint32_t* branches)
{
  fleet_paths_host(n, V, fields, slot, vtx, code, count, potential, off, nullptr, counters);   // count = hops for now
  uint32_t* hops = new uint32_t[n ? n : 1];
  for (uint32_t i = 0; i < n; ++i) { hops[i] = count[i]; count[i] = plan_pose_count(hops[i]); }
  fleet_scan_host(n, count, off);
  const unsigned long long total = off[n];
  uint32_t* ids = new uint32_t[total ? total : 1];
  float* lengths = new float[total ? total : 1];
  for (uint32_t i = 0; i < n; ++i) if (hops[i]) fleet_write(fields[slot[i]], vtx[i], hops[i], ids + off[i]);
  PlanView Q; Q.n = n; Q.V = V; Q.xyz = xyz; Q.vn = vn; Q.start = start; Q.goal = goal; Q.slot = slot; Q.count = count; Q.ids = ids; Q.off = off;
  for (unsigned long long g = 0; g < total; ++g) {
    int branch = 0;
    double p[kPoseDoubles];
    lengths[g] = plan_pose(Q, g, p, &branch);
    if (poses) for (int c = 0; c < kPoseDoubles; ++c) poses[kPoseDoubles * g + c] = p[c];
    if (branches) branches[branch] += 1u;
  }
  for (uint32_t i = 0; i < n; ++i) cost[i] = plan_cost(lengths, off[i], count[i]);
  delete[] hops; delete[] ids; delete[] lengths;
}
#endif

#if defined(__HIPCC__)

// count[i] = the poses of robot i (len[i] hops); block sums for the scan
__global__ __launch_bounds__(kFleetBlock) void k_plan_count(uint32_t n, const uint32_t* __restrict__ len, uint32_t* __restrict__ count,
                                                           unsigned long long* __restrict__ bsum)
{
  const uint32_t i = blockIdx.x * kFleetBlock + threadIdx.x;
  uint32_t c = 0u;
  if (i < n) { c = plan_pose_count(len[i]); count[i] = c; }
  fleet_block_sum(c, bsum);
}

// one lane per packed pose; poses: null for the lengths alone (the sizing call)
__global__ __launch_bounds__(kFleetBlock) void k_plan_poses(PlanView Q, unsigned long long total, double* __restrict__ poses, float* __restrict__ lengths)
{
  const unsigned long long g = (unsigned long long)blockIdx.x * kFleetBlock + threadIdx.x;
  if (g >= total) return;
  if (!poses) { lengths[g] = plan_pose(Q, g, nullptr); return; }
  double p[kPoseDoubles];
  lengths[g] = plan_pose(Q, g, p);
  double* out = poses + kPoseDoubles * g;
  MNAV_UNROLL
  for (int c = 0; c < kPoseDoubles; ++c) out[c] = p[c];
}

__global__ __launch_bounds__(kFleetBlock) void k_plan_cost(uint32_t n, const uint32_t* __restrict__ count, const unsigned long long* __restrict__ off,
                                                          const float* __restrict__ lengths, double* __restrict__ cost)
{
  const uint32_t i = blockIdx.x * kFleetBlock + threadIdx.x;
  if (i < n) cost[i] = plan_cost(lengths, off[i], count[i]);
}

// One wave per robot of the chunk: its scratch row (walk order) into the poses [off, off + len) of the packed output.  A
// row that would end beyond out_cap poses is left out (the call then reports the size it needs).
__global__ __launch_bounds__(64) void k_walk_poses(uint32_t cap, uint32_t F, const float* __restrict__ row_pos, const uint32_t* __restrict__ row_face,
                                                  const uint32_t* __restrict__ slot, const uint32_t* __restrict__ len, const unsigned long long* __restrict__ off,
                                                  const float* __restrict__ face_normals, const double* __restrict__ goal_pose, double* __restrict__ poses,
                                                  unsigned long long out_cap)
{
  const uint32_t j = blockIdx.x;
  WalkRow R; R.pos = row_pos + 3 * (size_t)cap * j; R.face = row_face + (size_t)cap * j; R.m = len[j] < cap ? len[j] : cap;
  const unsigned long long o = off[j];
  if (o + R.m > out_cap) return;
  const GPtr<const double> goal = goal_pose + kPoseDoubles * (size_t)slot[j];
  for (uint32_t q = threadIdx.x; q < R.m; q += 64u) {
    double p[kPoseDoubles];
    walk_pose(R, q, face_normals, F, goal, p);
    double* out = poses + kPoseDoubles * (o + q);
    MNAV_UNROLL
    for (int c = 0; c < kPoseDoubles; ++c) out[c] = p[c];
  }
}

__global__ __launch_bounds__(kFleetBlock) void k_walk_cost(uint32_t n, uint32_t cap, const float* __restrict__ row_pos, const uint32_t* __restrict__ len,
                                                          double* __restrict__ cost)
{
  const uint32_t j = blockIdx.x * kFleetBlock + threadIdx.x;
  if (j >= n) return;
  WalkRow R; R.pos = row_pos + 3 * (size_t)cap * j; R.face = nullptr; R.m = len[j] < cap ? len[j] : cap;
  cost[j] = walk_cost(R);
}

// buffers of the last fleet plans call (the per-robot and per-plan buffers of State serve it too)
struct PlanState {
  mnav::DevBuf<uint32_t> count; mnav::DevBuf<double> cost; size_t cap = 0;          // per robot
  mnav::DevBuf<float> goal; mnav::DevBuf<double> goal_pose; size_t slots_cap = 0;   // per plan
  mnav::DevBuf<uint32_t> ids; mnav::DevBuf<float> lengths; size_t scratch_cap = 0;  // per pose: never downloaded
  mnav::DevBuf<double> poses; size_t poses_cap = 0;                                 // packed poses
};

#endif  // __HIPCC__

}  // namespace mnav_fleet
