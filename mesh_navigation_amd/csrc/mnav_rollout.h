// mnav_rollout.h -- device rollouts (mnav_follow_rollout): many controller ticks per call for a batch of robots whose
// state stays resident.  The loop is Move Base Flex's: computeVelocityCommands (mnav_follow.h's fol_tick, bit for bit one
// mnav_follow_batch call), then isGoalReached (mesh_controller.cpp:172-177), then the robot moves -- here a unicycle
// integrated with the host libm's float cos / sin (mnav_eval.h cosf_ref / sinf_ref), so that device, host mirror and the
// Python model of the tests agree by bits.  Everything is built from the MNAV_HD pieces that already exist; the one new
// rule is rol_after_tick, which the device passes (through Tick::finish) and the host mirror rol_run call.
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
// Device shape: tick-synchronous over the resident state, three kernels per tick on the context's stream, which are
// passes A, B and C of mnav_follow.h over another policy (Tick): a robot has a tick while it is RUNNING, and the tick's
// Result goes through rol_after_tick into its row instead of into an output row.  Unlike the one-tick call nothing goes
// to the host between ticks: both list passes size themselves from the list lengths on the device (grid-stride), the
// lookup index exists before the first tick, and every tick has its own row of 8 counters (cleared once up front), which
// are the lists' lengths and the statistics at once (rol_fold_counters makes a call's Stats of them on the host).  A
// robot's row is written by exactly one pass per tick; passes hand over through vector stores and vector atomics at kernel
// boundaries.  mnav_fleet_rollout without start ticks runs these kernels too (mnav_rollout_capi.h, rollout_run).
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

// steps 2 to 5 (and the count of step 1) for a RUNNING robot whose tick gave R; false: the robot stopped
MNAV_HD bool rol_arrive(State& S, const mnav_fol::Result& R, const Params& P, W3 goal_pos, W3 goal_dir)
{
  S.ticks += 1;
  if (R.code == mnav_fol::kOutOfMap) { S.status = kOutOfMap; S.face = kNone; return false; }
  S.pos = R.pos; S.face = R.face;
  if (P.have_goal) {
    const float gd = mnav::w3_length(mnav::w3_sub(goal_pos, S.pos));                                // :175
    const float ang = mnav::acosf_ref(mnav::w3_dot(goal_dir, S.dir));                              // :176
    S.min_goal_dist = gd < S.min_goal_dist ? gd : S.min_goal_dist;
    if (gd <= P.dist_tolerance && ang <= P.angle_tolerance) { S.status = kReached; return false; } // :177
  }
  if (R.code == mnav_fol::kNoField) { S.status = kNoField; return false; }
  return true;
}

// step 6 under the command (lin, ang) at the tick's cost; the rollouts pass the follower's own command, mnav_sample.h a
// candidate's
MNAV_HD void rol_step(State& S, double lin, double ang, float cost, const Params& P)
{
  const double step = lin * P.dt;
  S.travel += step;
  S.cost_integral += (double)cost * P.dt;
  S.pos = mnav::w3((float)((double)S.pos.x + (double)S.dir.x * step), (float)((double)S.pos.y + (double)S.dir.y * step),
                   (float)((double)S.pos.z + (double)S.dir.z * step));
  const float th = (float)(ang * P.dt);
  const float c = mnav::cosf_ref(th), s = mnav::sinf_ref(th);
  const W3 k = mnav::w3_cross(S.up, S.dir);
  const float h = mnav::w3_dot(S.up, S.dir) * (1.0f - c);
  S.dir = mnav::w3_normalized(mnav::w3_add(mnav::w3_add(mnav::w3_scale(S.dir, c), mnav::w3_scale(k, s)), mnav::w3_scale(S.up, h)));
}

// steps 2 to 6 (and the count of step 1) for a RUNNING robot whose tick gave R
MNAV_HD void rol_after_tick(State& S, const mnav_fol::Result& R, const Params& P, W3 goal_pos, W3 goal_dir)
{
  if (rol_arrive(S, R, P, goal_pos, goal_dir)) rol_step(S, R.lin, R.ang, R.cost, P);
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

// What a call tells of itself afterwards (mnav_rollout_stats; the first fields of mnav_fleet_rollout_stats).  The context
// keeps one record per entry point; `= {}` is the reset.
struct Stats {
  uint32_t final_status[4] = { 0, 0, 0, 0 }, built_index = 0; uint64_t robot_ticks = 0, stayed = 0, neighbour = 0, global = 0;
  float ms_kernels = 0.f, ms_total = 0.f;
};
constexpr int kCounterWords = 8;                                          // a tick's counter row (mnav_follow.h, kCounters)

// The counter rows of the `ticks` ticks a call of n robots ran, folded into its statistics, on the host (plain C++; not
// behind the host mirrors' guard, since the device pass of the compiler reads the caller too).  Words 0 and 1 of a row are
// the work lists' lengths and tell nothing; a robot that has not stopped is still running.
inline void rol_fold_counters(const uint32_t* cnt, size_t ticks, uint32_t n, Stats& S)
{
  uint64_t sum[kCounterWords] = {};
  for (size_t t = 0; t < ticks; ++t)
    for (int k = 2; k < kCounterWords; ++k) sum[k] += cnt[(size_t)kCounterWords * t + k];
  S.stayed = sum[2]; S.neighbour = sum[3]; S.global = sum[4];
  S.final_status[kReached] = (uint32_t)sum[5]; S.final_status[kOutOfMap] = (uint32_t)sum[6]; S.final_status[kNoField] = (uint32_t)sum[7];
  S.final_status[kRunning] = n - (uint32_t)(sum[5] + sum[6] + sum[7]);
  S.robot_ticks = sum[2] + sum[3] + sum[4] + sum[6];                  // every tick of a robot ends in a face or out of the map
}

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

using mnav_fol::kCounters;
using mnav_fol::kStayBlock;

// the resident state (one row per robot, read and written in place; pos, dir, up, face: the context's staging), the
// counter rows of the call (Robots::cnt: the first row) and the optional trace (robot-major, trace_rows rows per robot)
struct Batch : mnav_fol::Robots {
  float* pos; float* dir; const float* up; uint32_t* face;
  int32_t* status; uint32_t* ticks; double* travel; double* cost_integral; float* min_goal_dist;
  const float* goal_pos; const float* goal_dir;                                                                 // null without goals
  float* trace; uint32_t trace_rows;
};

// The robots of one tick as the passes of mnav_follow.h see them: a robot has a tick while it is RUNNING, a stopped one
// repeats its position in the trace, and the tick's Result goes through rol_after_tick into the row (`up` and the plan
// never change).  A status is a kEnd* of mnav_follow.h.
struct Tick : Batch {
  Params P; uint32_t trace_row;                                       // trace_row kNone: this tick leaves no row

  __device__ __forceinline__ Tick(const Batch& B, const Params& P_, uint32_t tick, uint32_t trace_row_) : Batch(B), P(P_), trace_row(trace_row_)
  {
    cnt += (size_t)kCounters * tick;
  }
  __device__ __forceinline__ bool first(uint32_t ic, uint32_t& f, W3& p) const
  {
    const int32_t st = status[ic];
    f = face[ic]; p = mnav::w3_load(pos + 3 * (size_t)ic);
    return st == kRunning;
  }
  __device__ __forceinline__ void trace_at(uint32_t i, W3 p) const
  {
    if (trace_row == kNone) return;
    float* row = trace + 3 * ((size_t)i * trace_rows + trace_row);
    row[0] = p.x; row[1] = p.y; row[2] = p.z;
  }
  __device__ __forceinline__ void idle(uint32_t i, W3 p) const { trace_at(i, p); }   // a stopped robot repeats its position
  __device__ __forceinline__ State load(uint32_t i, uint32_t f, W3 p) const
  {
    State S;
    S.pos = p; S.dir = mnav::w3_load(dir + 3 * (size_t)i); S.up = mnav::w3_load(up + 3 * (size_t)i);
    S.face = f; S.status = status[i]; S.ticks = ticks[i]; S.travel = travel[i]; S.cost_integral = cost_integral[i];
    S.min_goal_dist = min_goal_dist[i];
    return S;
  }
  __device__ __forceinline__ int finish(uint32_t i, State& S, const mnav_fol::Result& R) const
  {
    const W3 zero = mnav::w3(0, 0, 0);
    rol_after_tick(S, R, P, P.have_goal ? mnav::w3_load(goal_pos + 3 * (size_t)i) : zero, P.have_goal ? mnav::w3_load(goal_dir + 3 * (size_t)i) : zero);
    pos[3 * (size_t)i] = S.pos.x; pos[3 * (size_t)i + 1] = S.pos.y; pos[3 * (size_t)i + 2] = S.pos.z;
    dir[3 * (size_t)i] = S.dir.x; dir[3 * (size_t)i + 1] = S.dir.y; dir[3 * (size_t)i + 2] = S.dir.z;
    face[i] = S.face; status[i] = S.status; ticks[i] = S.ticks; travel[i] = S.travel; cost_integral[i] = S.cost_integral;
    min_goal_dist[i] = S.min_goal_dist;
    trace_at(i, S.pos);
    return S.status;
  }
};
static_assert(kRunning == mnav_fol::kEndRunning && kReached == mnav_fol::kEndReached && kOutOfMap == mnav_fol::kEndOutOfMap && kNoField == mnav_fol::kEndNoField,
              "a rollout status is how a tick ended");

__global__ __launch_bounds__(kStayBlock) void k_rollout_stay(Batch B, WalkMesh M, mnav_fol::Config C, Params P, uint32_t tick, uint32_t trace_row)
{
  mnav_fol::fol_pass_stay(Tick(B, P, tick, trace_row), M, C);
}

__global__ __launch_bounds__(64) void k_rollout_search(Batch B, WalkMesh M, mnav_fol::Config C, Params P, uint32_t tick, uint32_t trace_row)
{
  __shared__ uint32_t list[mnav::kWalkScratchWords];
  mnav_fol::fol_pass_search(Tick(B, P, tick, trace_row), M, C, list);
}

// (the second list's length is the tick's cnt[1], final when pass B has ended: nothing goes to the host)
__global__ __launch_bounds__(mnav_loc::kLocBlock) void k_rollout_global(Batch B, WalkMesh M, mnav_fol::Config C, Params P, mnav_loc::Index I, uint32_t tick,
                                                                       uint32_t trace_row)
{
  __shared__ uint32_t s_node[mnav_loc::kStack * mnav_loc::kLocBlock];
  __shared__ float s_bound[mnav_loc::kStack * mnav_loc::kLocBlock];
  const Tick T(B, P, tick, trace_row);
  mnav_fol::fol_pass_global(T, M, C, I, T.cnt[1] < T.n ? T.cnt[1] : T.n, s_node, s_bound);
}

static_assert(kCounterWords == kCounters, "rol_fold_counters reads the rows the passes write");

// what a rollout keeps on the device beside the context's staging (grown on demand, kept between calls; both entry points
// use it, a call uploads every input at entry): the rest of the robots' rows, goals, counter rows, trace
struct Dev {
  mnav::DevBuf<float> min_goal_dist, goal_pos, goal_dir, trace; mnav::DevBuf<double> travel, cost_integral;
  mnav::DevBuf<uint32_t> ticks, cnt; mnav::DevBuf<int32_t> status;
  size_t cap = 0, cnt_cap = 0, trace_cap = 0;
};

#endif  // __HIPCC__

}  // namespace mnav_rol
