// mnav_rollout.h -- device rollouts (mnav_follow_rollout): many controller ticks per call for a batch of robots whose
// state stays resident.  The loop is Move Base Flex's: computeVelocityCommands (mnav_follow.h's fol_tick, bit for bit one
// mnav_follow_batch call), then isGoalReached (mesh_controller.cpp:172-177), then the robot moves -- here a unicycle
// integrated with the host libm's float cos / sin (mnav_eval.h cosf_ref / sinf_ref), so that device, host mirror and the
// Python model of the tests agree by bits.  Everything is built from the MNAV_HD pieces that already exist; the one new
// rule is rol_after_tick, which every device pass and the host mirror rol_run call.
//
// One tick of a RUNNING robot, in this order and these types, no contraction:
//   1  R = fol_tick(pos, dir, up, face); ticks += 1
//   2  R.code == OUT_OF_MAP: status OUT_OF_MAP, face NONE, pos unchanged, the robot stops
//   3  pos = R.pos, face = R.face (the given position for a robot that stayed on its face, else the projection)
//   4  with goals: gd = |goal_pos - pos|, ang = acosf(goal_dir . dir) (:175-176, unqualified acos on a float, as :232);
//      min_goal_dist = min(min_goal_dist, gd); gd <= (float)dist_tolerance && ang <= (float)angle_tolerance: REACHED, stops
//      (a NaN angle -- a dot product rounded above 1 -- is not reached, as in the reference)
//   5  R.code == NO_FIELD: status NO_FIELD, the robot stops
//   6  step = R.lin * dt (double); travel += step; cost_integral += (double)R.cost * dt;
//      pos.c = (float)((double)pos.c + (double)dir.c * step); th = (float)(R.ang * dt);
//      dir = normalized(dir * cos th + (up x dir) * sin th + up * ((up . dir) * (1 - cos th)))   (Rodrigues, float)
// A robot that is not RUNNING is left untouched by later ticks.
//
// Device shape: tick-synchronous over the resident state, three kernels per tick on the context's stream that mirror
// passes A, B and C of mnav_follow.h (k_rollout_stay: one lane per robot, stay test + tail + rol_after_tick fused;
// k_rollout_search: one wave per listed robot; k_rollout_global: one lane per listed robot).  Unlike the one-tick call
// nothing goes to the host between ticks: both list passes size themselves from the list lengths on the device
// (grid-stride), the lookup index exists before the first tick, and every tick has its own row of 8 counters (cleared
// once up front), which are the lists' lengths and the statistics at once.  A robot's row is written by exactly one pass
// per tick; passes hand over through vector stores and vector atomics at kernel boundaries.
#pragma once
#include <cmath>
#include <cstdint>

#include "mnav_follow.h"

namespace mnav_rol {

using mnav::kNone;
using mnav::W3;
using mnav::WalkField;
using mnav::WalkMesh;

enum : int { kRunning = 0, kReached = 1, kOutOfMap = 2, kNoField = 3 };   // MNAV_ROLLOUT_*, include/mnav.h
constexpr uint32_t kBlockTicks = 256;                                     // ticks between two looks at the cancel flag
constexpr uint32_t kMaxTicks = 100000;

struct State {
  W3 pos, dir, up; uint32_t face; int32_t status; uint32_t ticks; double travel, cost_integral; float min_goal_dist;
};
// what does not change over a call; goal_pos / goal_dir are per robot
struct Params { double dt; float dist_tolerance, angle_tolerance; bool have_goal; };

MNAV_HD State rol_start(W3 pos, W3 dir, W3 up, uint32_t face)
{
  State S;
  S.pos = pos; S.dir = dir; S.up = up; S.face = face; S.status = kRunning; S.ticks = 0; S.travel = 0.0; S.cost_integral = 0.0; S.min_goal_dist = INFINITY;
  return S;
}

// steps 2 to 6 (and the count of step 1) for a RUNNING robot whose tick gave R
MNAV_HD void rol_after_tick(State& S, const mnav_fol::Result& R, const Params& P, W3 goal_pos, W3 goal_dir)
{
  S.ticks += 1;
  if (R.code == mnav_fol::kOutOfMap) { S.status = kOutOfMap; S.face = kNone; return; }
  S.pos = R.pos; S.face = R.face;
  if (P.have_goal) {
    const float gd = mnav::w3_length(mnav::w3_sub(goal_pos, S.pos));                                // :175
    const float ang = mnav::acosf_ref(mnav::w3_dot(goal_dir, S.dir));                              // :176
    S.min_goal_dist = gd < S.min_goal_dist ? gd : S.min_goal_dist;
    if (gd <= P.dist_tolerance && ang <= P.angle_tolerance) { S.status = kReached; return; }       // :177
  }
  if (R.code == mnav_fol::kNoField) { S.status = kNoField; return; }
  const double step = R.lin * P.dt;
  S.travel += step;
  S.cost_integral += (double)R.cost * P.dt;
  S.pos = mnav::w3((float)((double)S.pos.x + (double)S.dir.x * step), (float)((double)S.pos.y + (double)S.dir.y * step),
                   (float)((double)S.pos.z + (double)S.dir.z * step));
  const float th = (float)(R.ang * P.dt);
  const float c = mnav::cosf_ref(th), s = mnav::sinf_ref(th);
  const W3 k = mnav::w3_cross(S.up, S.dir);
  const float h = mnav::w3_dot(S.up, S.dir) * (1.0f - c);
  S.dir = mnav::w3_normalized(mnav::w3_add(mnav::w3_add(mnav::w3_scale(S.dir, c), mnav::w3_scale(k, s)), mnav::w3_scale(S.up, h)));
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The host mirror, serially: `ticks` ticks of one robot from S on (ticks x fol_tick + rol_after_tick).  trace: null, or
// ticks / trace_stride rows of 3 floats, a row after every trace_stride-th tick (a stopped robot repeats its position);
// how_hist: null, or 5 counters of the ticks' `how`.  `list`: kWalkScratchWords words.
template <class Stack>
inline void rol_run(const WalkMesh& M, const mnav_loc::Index& I, Stack& st, const WalkField& Fd, const float* costs, const mnav_fol::Config& C, const Params& P,
                    W3 goal_pos, W3 goal_dir, State& S, uint32_t ticks, uint32_t trace_stride, float* trace, uint32_t* list, uint64_t* how_hist)
{
  for (uint32_t t = 1; t <= ticks; ++t) {
    if (S.status == kRunning) {
      const mnav_fol::Result R = mnav_fol::fol_tick(M, I, st, Fd, costs, C, S.pos, S.dir, S.up, S.face, list);
      if (how_hist) ++how_hist[R.how];
      rol_after_tick(S, R, P, goal_pos, goal_dir);
    }
    if (trace && trace_stride && t % trace_stride == 0) {
      float* row = trace + 3 * (size_t)(t / trace_stride - 1);
      row[0] = S.pos.x; row[1] = S.pos.y; row[2] = S.pos.z;
    }
  }
}
#endif

// The call's tick loop on the host, in blocks of at most kBlockTicks: run_block(first_tick, n_ticks) enqueues a block and waits for it
// (non-zero: an error, passed on), then `cancelled()` is looked at once.  Returns 0, 1 when the flag ended the loop (also
// after the last block: the caller asked to stop), or run_block's error; *done = ticks run.
template <class RunBlock, class Cancelled>
inline int rol_blocks(uint32_t ticks, RunBlock run_block, Cancelled cancelled, uint32_t* done)
{
  *done = 0;
  while (*done < ticks) {
    const uint32_t nt = ticks - *done < kBlockTicks ? ticks - *done : kBlockTicks;
    const int rc = run_block(*done, nt);
    if (rc) return rc;
    *done += nt;
    if (cancelled()) return 1;
  }
  return 0;
}

#if defined(__HIPCC__)

constexpr int kCounters = 8;   // per tick: neighbour list length, global list length, stayed, neighbour, global, reached, out of map, no field
constexpr int kStayBlock = 256;

// the resident state (one row per robot, read and written in place), the per-slot vector maps, the two work lists, the
// counter rows of the call and the optional trace (robot-major, trace_rows rows per robot)
struct Batch {
  uint32_t n;
  float* pos; float* dir; const float* up; uint32_t* face; const uint32_t* slot; const uint32_t* seed_face;   // seed_face: may be null
  int32_t* status; uint32_t* ticks; double* travel; double* cost_integral; float* min_goal_dist;
  const float* goal_pos; const float* goal_dir;                                                                 // null without goals
  const float* const* vecmaps; const float* costs;
  uint32_t* nb_list; uint32_t* gl_list; uint32_t* cnt;
  float* trace; uint32_t trace_rows;
};

__device__ __forceinline__ State rol_load(const Batch& B, uint32_t i)
{
  State S;
  S.pos = mnav::w3_load(B.pos + 3 * (size_t)i); S.dir = mnav::w3_load(B.dir + 3 * (size_t)i); S.up = mnav::w3_load(B.up + 3 * (size_t)i);
  S.face = B.face[i]; S.status = B.status[i]; S.ticks = B.ticks[i]; S.travel = B.travel[i]; S.cost_integral = B.cost_integral[i];
  S.min_goal_dist = B.min_goal_dist[i];
  return S;
}

__device__ __forceinline__ void rol_trace(const Batch& B, uint32_t i, uint32_t trace_row, W3 pos)
{
  if (trace_row == kNone) return;
  float* row = B.trace + 3 * ((size_t)i * B.trace_rows + trace_row);
  row[0] = pos.x; row[1] = pos.y; row[2] = pos.z;
}

// rol_after_tick on robot i's row, the row and its trace entry written back (`up` and the plan never change)
__device__ __forceinline__ int rol_finish(const Batch& B, const Params& P, uint32_t i, State& S, const mnav_fol::Result& R, uint32_t trace_row)
{
  const W3 zero = mnav::w3(0, 0, 0);
  rol_after_tick(S, R, P, P.have_goal ? mnav::w3_load(B.goal_pos + 3 * (size_t)i) : zero, P.have_goal ? mnav::w3_load(B.goal_dir + 3 * (size_t)i) : zero);
  B.pos[3 * (size_t)i] = S.pos.x; B.pos[3 * (size_t)i + 1] = S.pos.y; B.pos[3 * (size_t)i + 2] = S.pos.z;
  B.dir[3 * (size_t)i] = S.dir.x; B.dir[3 * (size_t)i + 1] = S.dir.y; B.dir[3 * (size_t)i + 2] = S.dir.z;
  B.face[i] = S.face; B.status[i] = S.status; B.ticks[i] = S.ticks; B.travel[i] = S.travel; B.cost_integral[i] = S.cost_integral;
  B.min_goal_dist[i] = S.min_goal_dist;
  rol_trace(B, i, trace_row, S.pos);
  return S.status;
}

// the counters of the robots a wave finished this tick (the whole wave must call this)
__device__ __forceinline__ void rol_count(uint32_t* cnt, bool done, int how, int status)
{
  const unsigned long long b[6] = { __ballot(done && how == mnav_fol::kHowStay), __ballot(done && how == mnav_fol::kHowNeighbour),
                                    __ballot(done && (how == mnav_fol::kHowFirst || how == mnav_fol::kHowGlobal)), __ballot(done && status == kReached),
                                    __ballot(done && status == kOutOfMap), __ballot(done && status == kNoField) };
  if ((threadIdx.x & 63u) == 0)
    for (int k = 0; k < 6; ++k) if (b[k]) atomicAdd(&cnt[2 + k], (uint32_t)__popcll(b[k]));
}

// Pass A: one lane per robot.  The row's first loads go to a clamped index, unconditionally.
__global__ __launch_bounds__(kStayBlock) void k_rollout_stay(Batch B, WalkMesh M, mnav_fol::Config C, Params P, uint32_t tick, uint32_t trace_row)
{
  const uint32_t i = blockIdx.x * kStayBlock + threadIdx.x;
  const uint32_t ic = i < B.n ? i : B.n - 1;
  uint32_t* cnt = B.cnt + (size_t)kCounters * tick;
  const int32_t status = B.status[ic];
  const uint32_t f = B.face[ic];
  const W3 p = mnav::w3_load(B.pos + 3 * (size_t)ic);
  int route = 0, how = mnav_fol::kHowNone, after = kRunning;                // route 1: neighbour search, 2: global search
  bool done = false;
  if (i < B.n) {
    if (status != kRunning) rol_trace(B, i, trace_row, p);              // a stopped robot repeats its position
    else if (f == kNone) route = 2;
    else {
      float bary[3];
      if (mnav_fol::fol_stay(M, p, f, C.max_search_distance, bary)) {
        State S = rol_load(B, i);
        const WalkField Fd = mnav_fol::fol_field(M, B.vecmaps[B.slot[i]], B.seed_face ? B.seed_face[i] : kNone);
        const mnav_fol::Result R = mnav_fol::fol_finish(M, Fd, B.costs, C, S.pos, S.dir, S.up, f, bary, mnav_fol::kHowStay, false);
        after = rol_finish(B, P, i, S, R, trace_row);
        how = R.how; done = true;
      } else route = 1;
    }
  }
  mnav_fol::fol_push(B.nb_list, &cnt[0], route == 1, i);
  mnav_fol::fol_push(B.gl_list, &cnt[1], route == 2, i);
  rol_count(cnt, done, how, after);
}

// Pass B: one wave per listed robot (grid-stride over the list, whose length pass A left in the tick's cnt[0])
__global__ __launch_bounds__(64) void k_rollout_search(Batch B, WalkMesh M, mnav_fol::Config C, Params P, uint32_t tick, uint32_t trace_row)
{
  __shared__ uint32_t list[mnav::kWalkScratchWords];
  uint32_t* cnt = B.cnt + (size_t)kCounters * tick;
  const uint32_t n_nb = cnt[0] < B.n ? cnt[0] : B.n;
  for (uint32_t j = blockIdx.x; j < n_nb; j += gridDim.x) {
    const uint32_t i = B.nb_list[j];
    const W3 p = mnav::w3_load(B.pos + 3 * (size_t)i);
    float bary[3];
    int status = mnav::kWalkLost;
    const uint32_t nf = mnav::walk_search_faces(M, p, B.face[i], (float)C.max_search_radius, (float)C.max_search_distance, bary, list, &status);
    if (threadIdx.x == 0) {
      if (nf == kNone) B.gl_list[atomicAdd(&cnt[1], 1u)] = i;           // (a robot is listed at most once per tick: the list holds n)
      else {
        State S = rol_load(B, i);
        const WalkField Fd = mnav_fol::fol_field(M, B.vecmaps[B.slot[i]], B.seed_face ? B.seed_face[i] : kNone);
        const mnav_fol::Result R = mnav_fol::fol_finish(M, Fd, B.costs, C, S.pos, S.dir, S.up, nf, bary, mnav_fol::kHowNeighbour, true);
        const int after = rol_finish(B, P, i, S, R, trace_row);
        atomicAdd(&cnt[3], 1u);
        if (after == kReached) atomicAdd(&cnt[5], 1u);
        if (after == kNoField) atomicAdd(&cnt[7], 1u);
      }
    }
    __syncthreads();                                                    // the next search reuses the list
  }
}

// Pass C: one lane per robot of the second list, whose length (the tick's cnt[1]) is final when pass B has ended:
// grid-stride in whole waves, so that the counters' ballots see every lane
__global__ __launch_bounds__(mnav_loc::kLocBlock) void k_rollout_global(Batch B, WalkMesh M, mnav_fol::Config C, Params P, mnav_loc::Index I, uint32_t tick,
                                                                       uint32_t trace_row)
{
  __shared__ uint32_t s_node[mnav_loc::kStack * mnav_loc::kLocBlock];
  __shared__ float s_bound[mnav_loc::kStack * mnav_loc::kLocBlock];
  uint32_t* cnt = B.cnt + (size_t)kCounters * tick;
  const uint32_t lane = threadIdx.x;
  const uint32_t n_gl = cnt[1] < B.n ? cnt[1] : B.n;
  for (uint32_t base = blockIdx.x * mnav_loc::kLocBlock; base < n_gl; base += gridDim.x * mnav_loc::kLocBlock) {
    const uint32_t j = base + lane;
    int how = mnav_fol::kHowNone, after = kRunning;
    if (j < n_gl) {
      uint64_t cand = 0;                                                // (distances evaluated: the lookup's statistic, not kept here)
      const uint32_t i = B.gl_list[j];
      State S = rol_load(B, i);
      mnav_loc::LdsStack st{ s_node, s_bound, lane, 0 };
      const WalkField Fd = mnav_fol::fol_field(M, B.vecmaps[B.slot[i]], B.seed_face ? B.seed_face[i] : kNone);
      const mnav_fol::Result R = mnav_fol::fol_global(M, I, st, Fd, B.costs, C, S.pos, S.dir, S.up, S.face == kNone ? mnav_fol::kHowFirst : mnav_fol::kHowGlobal, &cand);
      after = rol_finish(B, P, i, S, R, trace_row);
      how = R.how;
    }
    rol_count(cnt, j < n_gl, how, after);
  }
}

// buffers of the last call (grown on demand, kept between calls) and its statistics
struct Dev {
  mnav::DevBuf<float> pos, dir, up, min_goal_dist, goal_pos, goal_dir, trace; mnav::DevBuf<double> travel, cost_integral;
  mnav::DevBuf<uint32_t> face, slot, seed_face, ticks, nb_list, gl_list, cnt; mnav::DevBuf<int32_t> status;
  mnav::DevBuf<const float*> vecmaps; size_t cap = 0, slots_cap = 0, cnt_cap = 0, trace_cap = 0;
  mnav::Event ev[2]; bool have_ev = false;
  uint32_t final_status[4] = { 0, 0, 0, 0 }, built_index = 0; uint64_t robot_ticks = 0, stayed = 0, neighbour = 0, global = 0;
  float ms_kernels = 0.f, ms_total = 0.f;
};

#endif  // __HIPCC__

}  // namespace mnav_rol
