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
// (k_follow_stay) gives every robot ONE LANE: step 2 and the whole tail.  Robots that need a search are compacted into
// two work lists with wave-aggregated atomics.  Pass B (k_follow_search) gives each listed robot a WAVE for the
// breadth-first neighbour search (mnav_walk.h's wave version, list in LDS) and hands failures on to the second list.
// Pass C (k_follow_global) runs the exact nearest-vertex descent of mnav_locate.h, one lane per listed robot, and is the
// only pass that needs the lookup index: the host reads the two list lengths once after pass B and builds the index
// only if the second list is not empty.  A robot's outputs are written by exactly one pass, to its own row.
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

// one batch on the device: inputs, the per-slot vector maps, one output row per robot, the two work lists and
// cnt[0] / cnt[1] = their lengths, cnt[2..6] = robots that stayed / found a neighbour face / were found by a global
// search / are out of the map / have no field
struct Batch {
  uint32_t n;
  const float* pos; const float* dir; const float* up; const uint32_t* face_in; const uint32_t* slot; const uint32_t* seed_face;   // seed_face: may be null
  const float* const* vecmaps; const float* costs;
  int32_t* code; uint32_t* face; float* bary; float* pos_out; float* mesh_dir; float* cost; double* cmd; int32_t* how;
  uint32_t* nb_list; uint32_t* gl_list; uint32_t* cnt;
};
constexpr int kCounters = 8;
constexpr int kStayBlock = 256;

__device__ __forceinline__ WalkField fol_field_of(const Batch& B, const WalkMesh& M, uint32_t i)
{
  return fol_field(M, B.vecmaps[B.slot[i]], B.seed_face ? B.seed_face[i] : kNone);
}

__device__ __forceinline__ void fol_store(const Batch& B, uint32_t i, const Result& R)
{
  B.code[i] = R.code; B.how[i] = R.how; B.face[i] = R.face; B.cost[i] = R.cost;
  for (int k = 0; k < 3; ++k) B.bary[3 * (size_t)i + k] = R.bary[k];
  B.pos_out[3 * (size_t)i] = R.pos.x; B.pos_out[3 * (size_t)i + 1] = R.pos.y; B.pos_out[3 * (size_t)i + 2] = R.pos.z;
  B.mesh_dir[3 * (size_t)i] = R.mesh_dir.x; B.mesh_dir[3 * (size_t)i + 1] = R.mesh_dir.y; B.mesh_dir[3 * (size_t)i + 2] = R.mesh_dir.z;
  B.cmd[2 * (size_t)i] = R.lin; B.cmd[2 * (size_t)i + 1] = R.ang;
}

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
__device__ __forceinline__ void fol_count(uint32_t* cnt, bool done, int code, int how)
{
  const unsigned long long b[5] = { __ballot(done && how == kHowStay), __ballot(done && how == kHowNeighbour),
                                    __ballot(done && (how == kHowFirst || how == kHowGlobal)), __ballot(done && code == kOutOfMap),
                                    __ballot(done && code == kNoField) };
  if ((threadIdx.x & 63u) == 0)
    for (int k = 0; k < 5; ++k) if (b[k]) atomicAdd(&cnt[2 + k], (uint32_t)__popcll(b[k]));
}

// Pass A: one lane per robot
__global__ __launch_bounds__(kStayBlock) void k_follow_stay(Batch B, WalkMesh M, Config C)
{
  const uint32_t i = blockIdx.x * kStayBlock + threadIdx.x;
  int route = 0, code = kOk, how = kHowNone;                          // route 1: neighbour search, 2: global search
  if (i < B.n) {
    const uint32_t f = B.face_in[i];
    if (f == kNone) route = 2;
    else {
      const W3 p = mnav::w3_load(B.pos + 3 * (size_t)i);
      float bary[3];
      if (fol_stay(M, p, f, C.max_search_distance, bary)) {
        const Result R = fol_finish(M, fol_field_of(B, M, i), B.costs, C, p, mnav::w3_load(B.dir + 3 * (size_t)i), mnav::w3_load(B.up + 3 * (size_t)i), f,
                                    bary, kHowStay, false);
        fol_store(B, i, R);
        code = R.code; how = R.how;
      } else route = 1;
    }
  }
  fol_push(B.nb_list, &B.cnt[0], route == 1, i);
  fol_push(B.gl_list, &B.cnt[1], route == 2, i);
  fol_count(B.cnt, i < B.n && route == 0, code, how);
}

// Pass B: one wave per listed robot (grid-stride over the list, whose length pass A left in cnt[0])
__global__ __launch_bounds__(64) void k_follow_search(Batch B, WalkMesh M, Config C)
{
  __shared__ uint32_t list[mnav::kWalkScratchWords];
  const uint32_t n_nb = B.cnt[0] < B.n ? B.cnt[0] : B.n;
  for (uint32_t j = blockIdx.x; j < n_nb; j += gridDim.x) {
    const uint32_t i = B.nb_list[j];
    const W3 p = mnav::w3_load(B.pos + 3 * (size_t)i);
    float bary[3];
    int status = mnav::kWalkLost;
    const uint32_t nf = mnav::walk_search_faces(M, p, B.face_in[i], (float)C.max_search_radius, (float)C.max_search_distance, bary, list, &status);
    if (threadIdx.x == 0) {
      if (nf == kNone) B.gl_list[atomicAdd(&B.cnt[1], 1u)] = i;       // (a robot is listed at most once: the list holds n)
      else {
        const Result R = fol_finish(M, fol_field_of(B, M, i), B.costs, C, p, mnav::w3_load(B.dir + 3 * (size_t)i), mnav::w3_load(B.up + 3 * (size_t)i), nf,
                                    bary, kHowNeighbour, true);
        fol_store(B, i, R);
        atomicAdd(&B.cnt[3], 1u);
        if (R.code == kNoField) atomicAdd(&B.cnt[6], 1u);
      }
    }
    __syncthreads();                                                  // the next search reuses the list
  }
}

// Pass C: one lane per robot of the second list (n_gl: its length, read by the host after pass B)
__global__ __launch_bounds__(mnav_loc::kLocBlock) void k_follow_global(Batch B, WalkMesh M, Config C, mnav_loc::Index I, uint32_t n_gl)
{
  __shared__ uint32_t s_node[mnav_loc::kStack * mnav_loc::kLocBlock];
  __shared__ float s_bound[mnav_loc::kStack * mnav_loc::kLocBlock];
  const uint32_t lane = threadIdx.x;
  const uint32_t j = blockIdx.x * mnav_loc::kLocBlock + lane;
  int code = kOk, how = kHowNone;
  if (j < n_gl) {
    uint64_t cand = 0;                                                // (distances evaluated: the lookup's statistic, not kept here)
    const uint32_t i = B.gl_list[j];
    mnav_loc::LdsStack st{ s_node, s_bound, lane, 0 };
    const Result R = fol_global(M, I, st, fol_field_of(B, M, i), B.costs, C, mnav::w3_load(B.pos + 3 * (size_t)i), mnav::w3_load(B.dir + 3 * (size_t)i),
                                mnav::w3_load(B.up + 3 * (size_t)i), B.face_in[i] == kNone ? kHowFirst : kHowGlobal, &cand);
    fol_store(B, i, R);
    code = R.code; how = R.how;
  }
  fol_count(B.cnt, j < n_gl, code, how);
}

// buffers of the last call (grown on demand, kept between calls) and its counters
struct State {
  mnav::DevBuf<float> pos, dir, up, bary, pos_out, mesh_dir, cost; mnav::DevBuf<double> cmd;
  mnav::DevBuf<uint32_t> face_in, slot, seed_face, face, nb_list, gl_list, cnt; mnav::DevBuf<int32_t> code, how;
  mnav::DevBuf<const float*> vecmaps; size_t cap = 0, slots_cap = 0;
  mnav::Event ev[4]; bool have_ev = false;
  uint32_t stayed = 0, neighbour = 0, global = 0, lost = 0, no_field = 0, built_index = 0; float ms_kernels = 0.f, ms_total = 0.f;
};

#endif  // __HIPCC__

}  // namespace mnav_fol
