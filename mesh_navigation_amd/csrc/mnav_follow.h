// mnav_follow.h -- the vector-field follower on the device (mnav_follow_batch): one controller tick of
// mesh_controller::MeshController for a batch of robots over the vector maps the planners left resident.  Restates
// MeshController::computeVelocityCommands (mesh_controller.cpp:67-170) and naiveControl (:225-242) on the pieces that
// already have a single source: projectedBarycentricCoords / searchNeighbourFaces / directionAtPosition (mnav_walk.h),
// getNearestVertexHandle / searchContainingFace (mnav_locate.h) and the host libm's acosf (mnav_eval.h).
//
// Per robot, in the reference's order (`how` records which step found the face):
//   1 kHowFirst      no current face (:79): searchContainingFace; max_search_distance is passed and ignored there
//   2 kHowStay       the current face still holds the position: inside AND the SIGNED distance < max_search_distance
//                    (:109-111: float against double, no fabs -- a robot far BELOW its face stays on it); the position is kept
//   3 kHowNeighbour  searchNeighbourFaces(pos, face, max_search_radius, max_search_distance), both narrowed to float (:116-117)
//   4 kHowGlobal     searchContainingFace again (:129)
//   nothing found    kOutOfMap (:96, :142)
// Steps 1, 3 and 4 replace the position by its projection v0*b0 + v1*b1 + v2*b2 (util.h:182-183).  Then
// directionAtPosition on the plan's vector map (no vector / non-finite sum: kNoField, :151-156), mesh_dir = that vector
// divided by its float length (:157), cost = c0*b0 + c1*b1 + c2*b2 (mesh_map.cpp:658-672), naiveControl and the two
// std::min saturations in double (:161-162).  Everything is float32 / double in the reference's mix and operation order, no
// contraction: every output is the host's bit for bit, whatever pass of the device produced it.
//
// Departures (lvr2 and tf2 are not part of the reference tree, so what they do cannot be pinned):
//   * mesh_map::Normal's constructor (lvr2) may normalise mesh_dir a second time; here it is normalised once.
//   * poseToDirectionVector's quaternion-to-basis product (tf2) is not restated here: heading and up vector arrive as
//     vectors in the map frame and are used as given (the C++ MeshController converts the quaternion, in double).
//   * searchNeighbourFaces' list is unbounded in the reference; here it holds kWalkListCap faces, and a search that
//     would need more continues with step 4.
//   * The vector map has no "no entry" state on the device: an all-zero row is "no vector", and the three vertices of the
//     plan's seed face always count as having one (mnav::WalkField, as for the back-tracking walk).
//
// Device shape: the common tick is a robot still on its face -- one barycentric test and a dozen loads -- so pass A
// (fol_pass_stay) gives every robot ONE LANE: step 2 and the whole tail.  Robots that need a search are compacted into
// two work lists with wave-aggregated atomics.  Pass B (fol_pass_search) gives each listed robot a WAVE for the
// breadth-first neighbour search (mnav_walk.h's wave version, list in LDS) and hands failures on to the second list.
// Pass C (fol_pass_global) runs the exact nearest-vertex descent of mnav_locate.h, one lane per listed robot, and is the
// only pass that needs the lookup index.  A robot's row is written by exactly one pass.  The three passes are written
// once, as templates over the robots they serve, for two callers: this file's one-tick call (k_follow_*: the Result is
// stored as the robot's output row; the host reads the two list lengths once after pass B and builds the index only if
// the second list is not empty) and the rollout's tick (mnav_rollout.h, k_rollout_*).
#pragma once
#include <cmath>
#include <cstdint>

#include "mnav_locate.h"

namespace mnav_fol {

using mnav::kNone;
using mnav::W3;
using mnav::WalkField;
using mnav::WalkMesh;

// mesh_controller.h:193-200 (same layout as mnav_follow_config, include/mnav.h)
struct Config {
  double max_lin_velocity, max_ang_velocity, arrival_fading, ang_vel_factor, lin_vel_factor, max_angle, max_search_radius, max_search_distance;
};

enum : int { kOk = 0, kOutOfMap = 1, kNoField = 2 };
enum : int { kHowNone = 0, kHowFirst = 1, kHowStay = 2, kHowNeighbour = 3, kHowGlobal = 4 };

// what one tick produces; fields a tick did not reach stay zero (face: kNone)
struct Result {
  int code, how; uint32_t face; float bary[3]; W3 pos, mesh_dir; float cost; double lin, ang;
};

MNAV_HD Result fol_lost(W3 pos)
{
  Result R;
  R.code = kOutOfMap; R.how = kHowNone; R.face = kNone; R.bary[0] = R.bary[1] = R.bary[2] = 0.f;
  R.pos = pos; R.mesh_dir = mnav::w3(0, 0, 0); R.cost = 0.f; R.lin = 0.0; R.ang = 0.0;
  return R;
}

// :109-111
MNAV_HD bool fol_stay(const WalkMesh& M, W3 pos, uint32_t face, double max_search_distance, float bary[3])
{
  float dist;
  return mnav::walk_bary(M, pos, face, bary, &dist) && (double)dist < max_search_distance;
}

// the plan's field as the walk reads it; seed_face kNone: no seed rule
MNAV_HD WalkField fol_field(const WalkMesh& M, const float* vecmap, uint32_t seed_face)
{
  WalkField Fd;
  Fd.vecmap = vecmap;
  for (int k = 0; k < 3; ++k) Fd.seed_vs[k] = seed_face < M.F ? M.faces[3 * (size_t)seed_face + k] : kNone;
  return Fd;
}

// :225-242 and :161-162
MNAV_HD void fol_control(const Config& C, W3 mesh_dir, W3 dir, W3 up, double* lin, double* ang)
{
  const double pi = 3.14159265358979323846;
  const float phi = mnav::acosf_ref(mnav::w3_dot(mesh_dir, dir));                                 // :232
  const float sign_phi = mnav::w3_dot(mnav::w3_cross(mesh_dir, dir), up);                          // :233
  const float angular_velocity = copysignf((float)((double)phi * C.max_ang_velocity / pi), -sign_phi);   // :237
  const float max_angle = (float)(C.max_angle * pi / 180.0);                                       // :238
  const float max_linear = (float)C.max_lin_velocity;                                              // :239
  const float linear_velocity = phi <= max_angle ? max_linear - (phi * max_linear / max_angle) : 0.f;   // :240
  const double l = (double)linear_velocity * C.lin_vel_factor, a = (double)angular_velocity * C.ang_vel_factor;
  *lin = l < C.max_lin_velocity ? l : C.max_lin_velocity;                                          // :161 (std::min(a, b) = b < a ? b : a)
  *ang = a < C.max_ang_velocity ? a : C.max_ang_velocity;                                          // :162
}

// everything after the face is known (:146-162); `project`: steps 1, 3, 4 (:91, :125, :137)
MNAV_HD Result fol_finish(const WalkMesh& M, const WalkField& Fd, const float* costs, const Config& C, W3 pos, W3 dir, W3 up, uint32_t face,
                          const float bary[3], int how, bool project)
{
  Result R = fol_lost(pos);
  const uint32_t* vs = M.faces + 3 * (size_t)face;
  R.how = how; R.face = face;
  for (int k = 0; k < 3; ++k) R.bary[k] = bary[k];
  if (project)
    R.pos = mnav::w3_add(mnav::w3_add(mnav::w3_scale(mnav::w3_load(M.xyz + 3 * (size_t)vs[0]), bary[0]), mnav::w3_scale(mnav::w3_load(M.xyz + 3 * (size_t)vs[1]), bary[1])),
                         mnav::w3_scale(mnav::w3_load(M.xyz + 3 * (size_t)vs[2]), bary[2]));
  R.code = kNoField;
  const bool h0 = mnav::walk_has_vector(Fd, vs[0]), h1 = mnav::walk_has_vector(Fd, vs[1]), h2 = mnav::walk_has_vector(Fd, vs[2]);
  if (!(h0 || h1 || h2)) return R;                                                                 // mesh_map.cpp:634
  W3 vec = mnav::w3(0, 0, 0);
  if (h0) vec = mnav::w3_add(vec, mnav::w3_scale(mnav::w3_load(Fd.vecmap + 3 * (size_t)vs[0]), bary[0]));   // :637-639
  if (h1) vec = mnav::w3_add(vec, mnav::w3_scale(mnav::w3_load(Fd.vecmap + 3 * (size_t)vs[1]), bary[1]));
  if (h2) vec = mnav::w3_add(vec, mnav::w3_scale(mnav::w3_load(Fd.vecmap + 3 * (size_t)vs[2]), bary[2]));
  if (!mnav_loc::loc_finite(vec.x, vec.y, vec.z)) return R;                                        // :640
  R.mesh_dir = mnav::w3_normalized(vec);                                                           // mesh_controller.cpp:157
  R.cost = costs[vs[0]] * bary[0] + costs[vs[1]] * bary[1] + costs[vs[2]] * bary[2];               // :158
  fol_control(C, R.mesh_dir, dir, up, &R.lin, &R.ang);
  R.code = kOk;
  return R;
}

// searchContainingFace on the index, then the tail; `how` = kHowFirst or kHowGlobal
template <class Stack>
MNAV_HD Result fol_global(const WalkMesh& M, const mnav_loc::Index& I, Stack& st, const WalkField& Fd, const float* costs, const Config& C, W3 pos, W3 dir, W3 up,
                          int how, uint64_t* cand)
{
  const float p[3] = { pos.x, pos.y, pos.z };
  const uint64_t best = mnav_loc::loc_nearest(I, p, st, cand);
  float bary[3], dist;
  const uint32_t f = mnav_loc::loc_face(M, best == mnav_loc::kNoKey ? kNone : (uint32_t)best, p, bary, &dist);
  if (f == kNone) return fol_lost(pos);
  return fol_finish(M, Fd, costs, C, pos, dir, up, f, bary, how, true);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole tick in the reference's order, serially (the host mirror of the three passes; `list`: kWalkScratchWords words)
template <class Stack>
inline Result fol_tick(const WalkMesh& M, const mnav_loc::Index& I, Stack& st, const WalkField& Fd, const float* costs, const Config& C, W3 pos, W3 dir, W3 up,
                       uint32_t face_in, uint32_t* list)
{
  uint64_t cand = 0;
  if (face_in == kNone) return fol_global(M, I, st, Fd, costs, C, pos, dir, up, kHowFirst, &cand);       // :79-98
  float bary[3];
  if (fol_stay(M, pos, face_in, C.max_search_distance, bary)) return fol_finish(M, Fd, costs, C, pos, dir, up, face_in, bary, kHowStay, false);
  int status = mnav::kWalkLost;
  const uint32_t nf = mnav::walk_search_faces(M, pos, face_in, (float)C.max_search_radius, (float)C.max_search_distance, bary, list, &status);   // :116-117
  if (nf != kNone) return fol_finish(M, Fd, costs, C, pos, dir, up, nf, bary, kHowNeighbour, true);
  return fol_global(M, I, st, Fd, costs, C, pos, dir, up, kHowGlobal, &cand);                             // :129-138
}
#endif

#if defined(__HIPCC__)

// Both callers run the three passes below: the one-tick call (Batch, this file) and the rollout's tick (mnav_rol::Tick).
// What a pass knows of its robots is a small policy struct Q, passed by value.  Its base is Robots; beside that it has
//   bool first(ic, face, pos)   the first loads of row ic (a clamped index: see pass A); false: the robot has no tick
//   void idle(i, pos)           what a robot without a tick still gets
//   Row load(i, face, pos)      the whole row, given its first loads: pos, dir, up, face and whatever finish needs beside them
//   int finish(i, row, R)       what becomes of the tick's Result; returns how the tick ended (kEnd*)
// Nothing in a pass branches on the caller: the policy is the only difference.
struct Robots {
  uint32_t n;
  const uint32_t* slot; const uint32_t* seed_face;                    // seed_face: may be null
  const float* const* vecmaps; const float* costs;
  uint32_t* nb_list; uint32_t* gl_list; uint32_t* cnt;                // the two work lists; cnt: this tick's counter row
};
// A counter row: the two lists' lengths, then the robots that stayed / found a neighbour face / were found by a global
// search, and those whose tick ended reached / out of the map / without a field (1 + kEnd*)
constexpr int kCounters = 8;
constexpr int kStayBlock = 256;
enum : int { kEndRunning = 0, kEndReached = 1, kEndOutOfMap = 2, kEndNoField = 3 };   // = MNAV_ROLLOUT_*; the one-tick call never reaches

// one batch of the one-tick call: inputs and one output row per robot
struct Batch : Robots {
  const float* pos; const float* dir; const float* up; const uint32_t* face_in;
  int32_t* code; uint32_t* face; float* bary; float* pos_out; float* mesh_dir; float* cost; double* cmd; int32_t* how;

  struct Row { W3 pos, dir, up; uint32_t face; };
  __device__ __forceinline__ bool first(uint32_t ic, uint32_t& f, W3& p) const { f = face_in[ic]; p = mnav::w3_load(pos + 3 * (size_t)ic); return true; }
  __device__ __forceinline__ void idle(uint32_t, W3) const {}
  __device__ __forceinline__ Row load(uint32_t i, uint32_t f, W3 p) const
  {
    return Row{ p, mnav::w3_load(dir + 3 * (size_t)i), mnav::w3_load(up + 3 * (size_t)i), f };
  }
  __device__ __forceinline__ int finish(uint32_t i, const Row&, const Result& R) const
  {
    code[i] = R.code; how[i] = R.how; face[i] = R.face; cost[i] = R.cost;
    for (int k = 0; k < 3; ++k) bary[3 * (size_t)i + k] = R.bary[k];
    pos_out[3 * (size_t)i] = R.pos.x; pos_out[3 * (size_t)i + 1] = R.pos.y; pos_out[3 * (size_t)i + 2] = R.pos.z;
    mesh_dir[3 * (size_t)i] = R.mesh_dir.x; mesh_dir[3 * (size_t)i + 1] = R.mesh_dir.y; mesh_dir[3 * (size_t)i + 2] = R.mesh_dir.z;
    cmd[2 * (size_t)i] = R.lin; cmd[2 * (size_t)i + 1] = R.ang;
    return R.code == kOk ? kEndRunning : 1 + R.code;
  }
};

// append i to a work list for the lanes that `want`: one atomic per wave (the whole wave must call this)
__device__ __forceinline__ void fol_push(uint32_t* list, uint32_t* len, bool want, uint32_t i)
{
  const unsigned long long m = __ballot(want);
  if (!m) return;
  const int lane = (int)(threadIdx.x & 63u), leader = __ffsll((long long)m) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(len, (uint32_t)__popcll(m));
  base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);      // (leader is wave-uniform)
  if (want) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
}

// the outcome counters of the robots a wave finished (the whole wave must call this)
__device__ __forceinline__ void fol_count(uint32_t* cnt, bool done, int how, int end)
{
  const unsigned long long b[6] = { __ballot(done && how == kHowStay), __ballot(done && how == kHowNeighbour),
                                    __ballot(done && (how == kHowFirst || how == kHowGlobal)), __ballot(done && end == kEndReached),
                                    __ballot(done && end == kEndOutOfMap), __ballot(done && end == kEndNoField) };
  if ((threadIdx.x & 63u) == 0)
    for (int k = 0; k < 6; ++k) if (b[k]) atomicAdd(&cnt[2 + k], (uint32_t)__popcll(b[k]));
}

// the tail on robot i's row (f0, p: its first loads) once its face is known, and what the caller makes of it; returns how
// the tick ended
template <class Q>
__device__ __forceinline__ int fol_resolve(const Q& B, const WalkMesh& M, const Config& C, uint32_t i, uint32_t f0, W3 p, uint32_t face, const float bary[3],
                                           int how, bool project)
{
  auto S = B.load(i, f0, p);
  const WalkField Fd = fol_field(M, B.vecmaps[B.slot[i]], B.seed_face ? B.seed_face[i] : kNone);
  return B.finish(i, S, fol_finish(M, Fd, B.costs, C, S.pos, S.dir, S.up, face, bary, how, project));
}

// Pass A: one lane per robot (kStayBlock per workgroup).  The row's first loads are written at a clamped index, outside
// the bounds test; the row is completed from them, so nothing is read twice.
template <class Q>
__device__ __forceinline__ void fol_pass_stay(const Q& B, const WalkMesh& M, const Config& C)
{
  const uint32_t i = blockIdx.x * kStayBlock + threadIdx.x;
  uint32_t f; W3 p;
  const bool live = B.first(i < B.n ? i : B.n - 1, f, p);
  int route = 0, end = kEndRunning;                                   // route 1: neighbour search, 2: global search
  bool done = false;
  if (i < B.n) {
    float bary[3];
    if (!live) B.idle(i, p);
    else if (f == kNone) route = 2;
    else if (fol_stay(M, p, f, C.max_search_distance, bary)) { end = fol_resolve(B, M, C, i, f, p, f, bary, kHowStay, false); done = true; }
    else route = 1;
  }
  fol_push(B.nb_list, &B.cnt[0], route == 1, i);
  fol_push(B.gl_list, &B.cnt[1], route == 2, i);
  fol_count(B.cnt, done, kHowStay, end);
}

// Pass B: one wave per listed robot (grid-stride over the list, whose length pass A left in cnt[0]); list: kWalkScratchWords of LDS
template <class Q>
__device__ __forceinline__ void fol_pass_search(const Q& B, const WalkMesh& M, const Config& C, uint32_t* list)
{
  const uint32_t n_nb = B.cnt[0] < B.n ? B.cnt[0] : B.n;
  for (uint32_t j = blockIdx.x; j < n_nb; j += gridDim.x) {
    const uint32_t i = B.nb_list[j];
    uint32_t f; W3 p;
    B.first(i, f, p);                                                 // (its answer is not needed: a listed robot has a tick)
    float bary[3];
    int status = mnav::kWalkLost;
    const uint32_t nf = mnav::walk_search_faces(M, p, f, (float)C.max_search_radius, (float)C.max_search_distance, bary, list, &status);
    if (threadIdx.x == 0) {
      if (nf == kNone) B.gl_list[atomicAdd(&B.cnt[1], 1u)] = i;       // (a robot is listed at most once per tick: the list holds n)
      else {
        const int end = fol_resolve(B, M, C, i, f, p, nf, bary, kHowNeighbour, true);
        atomicAdd(&B.cnt[3], 1u);
        if (end != kEndRunning) atomicAdd(&B.cnt[4 + end], 1u);       // (a face was found: reached or no field)
      }
    }
    __syncthreads();                                                  // the next search reuses the list
  }
}

// Pass C: one lane per robot of the second list, whose length n_gl is final when pass B has ended: grid-stride in whole
// waves, so that the counters' ballots see every lane; s_node / s_bound: the lookup's LDS stacks
template <class Q>
__device__ __forceinline__ void fol_pass_global(const Q& B, const WalkMesh& M, const Config& C, const mnav_loc::Index& I, uint32_t n_gl, uint32_t* s_node,
                                                float* s_bound)
{
  const uint32_t lane = threadIdx.x;
  for (uint32_t base = blockIdx.x * mnav_loc::kLocBlock; base < n_gl; base += gridDim.x * mnav_loc::kLocBlock) {
    const uint32_t j = base + lane;
    int how = kHowNone, end = kEndRunning;
    if (j < n_gl) {
      uint64_t cand = 0;                                              // (distances evaluated: the lookup's statistic, not kept here)
      const uint32_t i = B.gl_list[j];
      uint32_t f; W3 p;
      B.first(i, f, p);                                               // (as in pass B)
      auto S = B.load(i, f, p);
      mnav_loc::LdsStack st{ s_node, s_bound, lane, 0 };
      const WalkField Fd = fol_field(M, B.vecmaps[B.slot[i]], B.seed_face ? B.seed_face[i] : kNone);
      const Result R = fol_global(M, I, st, Fd, B.costs, C, S.pos, S.dir, S.up, S.face == kNone ? kHowFirst : kHowGlobal, &cand);
      end = B.finish(i, S, R);
      how = R.how;
    }
    fol_count(B.cnt, j < n_gl, how, end);
  }
}

__global__ __launch_bounds__(kStayBlock) void k_follow_stay(Batch B, WalkMesh M, Config C) { fol_pass_stay(B, M, C); }

__global__ __launch_bounds__(64) void k_follow_search(Batch B, WalkMesh M, Config C)
{
  __shared__ uint32_t list[mnav::kWalkScratchWords];
  fol_pass_search(B, M, C, list);
}

// (n_gl: the second list's length, read by the host after pass B; the grid is exact, so the loop runs once)
__global__ __launch_bounds__(mnav_loc::kLocBlock) void k_follow_global(Batch B, WalkMesh M, Config C, mnav_loc::Index I, uint32_t n_gl)
{
  __shared__ uint32_t s_node[mnav_loc::kStack * mnav_loc::kLocBlock];
  __shared__ float s_bound[mnav_loc::kStack * mnav_loc::kLocBlock];
  fol_pass_global(B, M, C, I, n_gl, s_node, s_bound);
}

// The per-robot inputs of a follower call or a rollout on the device, the two work lists and the events around the
// passes: grown on demand, kept between calls, owned once by the context.  The two calls may share them because each
// uploads every input at entry, and a rollout is continued through the caller's arrays, never through what a call left
// here (the rollout advances pos, dir and face in place).
struct Staging {
  mnav::DevBuf<float> pos, dir, up; mnav::DevBuf<uint32_t> face, slot, seed_face, nb_list, gl_list; mnav::DevBuf<const float*> vecmaps;
  size_t cap = 0, slots_cap = 0;
  mnav::Event ev[4]; bool have_ev = false;
};

// outputs of the last call (grown on demand, kept between calls) and its counters
struct State {
  mnav::DevBuf<float> bary, pos_out, mesh_dir, cost; mnav::DevBuf<double> cmd; mnav::DevBuf<uint32_t> face, cnt; mnav::DevBuf<int32_t> code, how; size_t cap = 0;
  uint32_t stayed = 0, neighbour = 0, global = 0, lost = 0, no_field = 0, built_index = 0; float ms_kernels = 0.f, ms_total = 0.f;
};

#endif  // __HIPCC__

}  // namespace mnav_fol
