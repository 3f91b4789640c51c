// mnav_sample.h -- sampled rollouts (mnav_follow_sample): K candidate controls per robot, rolled out for `ticks` ticks on the
// device, scored on the planner's own potential field and picked per robot.  What a local planner asks at every control
// tick -- DWA or MPPI over the field -- answered where the fields live.
//
// A candidate is four doubles (lin_gain, lin_bias, ang_gain, ang_bias).  Row i * K + k is robot i under candidate k; a row
// is a rollout robot (mnav_rollout.h, State) plus pot, lethal and cmd0.  One tick of a RUNNING row is steps 1 to 6 of
// mnav_rollout.h with three differences (smp_after_tick, the one rule device, host mirror and tests share):
//   a  after step 3, whether R is OK or NO_FIELD: pot = d[v0]*b0 + d[v1]*b1 + d[v2]*b2 in float, left to right (the form of
//      fol_finish's cost), d the slot's resident potential, v0..2 the face's vertices in stored order, b = R.bary; and for
//      R OK: lethal |= !(R.cost < (float)lethal_cost), so a NaN cost is lethal
//   b  step 6 runs under u in place of R.lin / R.ang: u = gain * R.x; if (bias != 0) u += bias; u = u < max ? u : max (the
//      saturation of fol_control, idempotent on the follower's own command).  A zero bias is NOT added: x + 0.0 turns -0
//      into +0, and candidate (1, 0, 1, 0) must be the follower bit for bit.  The first tick of a row that reaches step 6
//      records cmd0 = (u_lin, u_ang) -- which can only be the row's first tick: a row that did not reach step 6 has stopped
//   c  at the end J = w_potential * (double)pot + w_cost * cost_integral + w_time * ((double)ticks * dt), double, left to
//      right; a row is feasible iff RUNNING or REACHED, not lethal and J finite.  pot starts at +inf.
// pot is the potential where the row's LAST tick found it, that is before that tick's step; one more step is one more tick.
// The pick per robot: the feasible row with the smallest (J, k) (smp_better: J by <, ties -- -0 against +0 is one -- to the
// smaller k), built from compares, counts and minima only.
//
// Device shape: k_sample_expand (one lane per row) writes the rows from the n uploaded robots; every tick runs the three
// passes of mnav_follow.h, unchanged, over the policy SampleTick (k_sample_stay / _search / _global); k_sample_score (one
// lane per row) writes J; k_sample_pick gives every robot a wave, lanes strided over its K rows, and reduces the associative
// (J, k) minimum over 64 lanes.  Expanded per row: what the pass bodies read by row index (pos, dir, face, slot, seed face).
// Per robot, indexed by row / K inside the policy: up, goal_pos, goal_dir.  Per slot: the potential pointer, beside the
// vector maps.  Rows are robot-major, so the lanes of a wave of the stay pass start on one robot's face.
#pragma once
#include <cmath>
#include <cstdint>

#include "mnav_rollout.h"

namespace mnav_smp {

using mnav::GPtr;
using mnav::kNone;
using mnav::W3;
using mnav::WalkField;
using mnav::WalkMesh;
using mnav_rol::kNoField;
using mnav_rol::kOutOfMap;
using mnav_rol::kReached;
using mnav_rol::kRunning;
using mnav_rol::Params;

constexpr uint32_t kMaxRows = 1u << 28;
constexpr int kCandDoubles = 4;
constexpr int kPickBlock = 256;                                        // k_sample_pick: four robots per workgroup

struct Cand { double lin_gain, lin_bias, ang_gain, ang_bias; };
// what the rule needs beside the rollout's Params: the two saturations of fol_control, (float)lethal_cost, the faces
struct Rule { double max_lin, max_ang; float lethal_cost; GPtr<const uint32_t> faces; uint32_t F; };
struct Weights { double w_potential, w_cost, w_time, dt; };
struct Row : mnav_rol::State { float pot; uint32_t lethal; double cmd0[2]; };
struct Pick { uint32_t k, n_feasible; double score, cmd[2]; };

MNAV_HD Row smp_start(W3 pos, W3 dir, W3 up, uint32_t face)
{
  Row W;
  static_cast<mnav_rol::State&>(W) = mnav_rol::rol_start(pos, dir, up, face);
  W.pot = INFINITY; W.lethal = 0; W.cmd0[0] = 0.0; W.cmd0[1] = 0.0;
  return W;
}

MNAV_HD Cand smp_cand(GPtr<const double> table, uint32_t k)
{
  return Cand{ table[kCandDoubles * (size_t)k], table[kCandDoubles * (size_t)k + 1], table[kCandDoubles * (size_t)k + 2], table[kCandDoubles * (size_t)k + 3] };
}

// difference b: a zero bias is skipped (x + 0.0 would make +0 of -0)
MNAV_HD double smp_command(double gain, double bias, double x, double cap)
{
  double u = gain * x;
  if (bias != 0) u += bias;
  return u < cap ? u : cap;
}

// difference a's potential; the loads stand at a clamped face, outside every branch on the tick's outcome
MNAV_HD float smp_potential(GPtr<const float> d, const Rule& Q, uint32_t face, const float bary[3])
{
  const size_t f = face < Q.F ? face : 0u;
  const uint32_t v0 = Q.faces[3 * f], v1 = Q.faces[3 * f + 1], v2 = Q.faces[3 * f + 2];
  return d[v0] * bary[0] + d[v1] * bary[1] + d[v2] * bary[2];
}

// steps 2 to 6 (and the count of step 1) for a RUNNING row whose tick gave R, under candidate c over the potential d
MNAV_HD void smp_after_tick(Row& W, const mnav_fol::Result& R, const Params& P, const Rule& Q, const Cand& c, GPtr<const float> d, W3 goal_pos, W3 goal_dir)
{
  const float pot = smp_potential(d, Q, R.face, R.bary);
  if (R.code != mnav_fol::kOutOfMap) W.pot = pot;                     // (nothing between step 3 and here reads it)
  if (R.code == mnav_fol::kOk) W.lethal |= !(R.cost < Q.lethal_cost) ? 1u : 0u;
  if (!mnav_rol::rol_arrive(W, R, P, goal_pos, goal_dir)) return;
  const double lin = smp_command(c.lin_gain, c.lin_bias, R.lin, Q.max_lin), ang = smp_command(c.ang_gain, c.ang_bias, R.ang, Q.max_ang);
  if (W.ticks == 1) { W.cmd0[0] = lin; W.cmd0[1] = ang; }
  mnav_rol::rol_step(W, lin, ang, R.cost, P);
}

// difference c
MNAV_HD double smp_score(float pot, double cost_integral, uint32_t ticks, const Weights& G)
{
  return G.w_potential * (double)pot + G.w_cost * cost_integral + G.w_time * ((double)ticks * G.dt);
}
MNAV_HD bool smp_finite(double x) { return x - x == 0.0; }
MNAV_HD bool smp_feasible(int32_t status, uint32_t lethal, double J) { return (status == kRunning || status == kReached) && !lethal && smp_finite(J); }
// whether feasible row (Jb, kb) goes before (Ja, ka); k kNone: no row yet.  Associative and commutative as a minimum.
MNAV_HD bool smp_better(double Ja, uint32_t ka, double Jb, uint32_t kb)
{
  return kb != kNone && (ka == kNone || Jb < Ja || (Jb == Ja && kb < ka));
}

// the pick of one robot over its K rows, serially (the host's form of k_sample_pick); cmd0: 2 doubles per row
MNAV_HD Pick smp_pick(uint32_t K, const int32_t* status, const uint8_t* lethal, const double* score, const double* cmd0)
{
  Pick B;
  B.k = kNone; B.n_feasible = 0; B.score = INFINITY; B.cmd[0] = 0.0; B.cmd[1] = 0.0;
  for (uint32_t k = 0; k < K; ++k) {
    if (!smp_feasible(status[k], lethal[k], score[k])) continue;
    ++B.n_feasible;
    if (smp_better(B.score, B.k, score[k], k)) { B.k = k; B.score = score[k]; }
  }
  if (B.k != kNone) { B.cmd[0] = cmd0[2 * (size_t)B.k]; B.cmd[1] = cmd0[2 * (size_t)B.k + 1]; }
  return B;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The host mirror, serially: `ticks` ticks of one row from W on (ticks x fol_tick + smp_after_tick).  how_hist: null, or 5
// counters of the ticks' `how`.  `list`: kWalkScratchWords words.
template <class Stack>
inline void smp_run(const WalkMesh& M, const mnav_loc::Index& I, Stack& st, const WalkField& Fd, const float* costs, const float* potential, const mnav_fol::Config& C,
                    const Params& P, const Rule& Q, const Cand& c, W3 goal_pos, W3 goal_dir, Row& W, uint32_t ticks, uint32_t* list, uint64_t* how_hist)
{
  for (uint32_t t = 0; t < ticks && W.status == kRunning; ++t) {
    const mnav_fol::Result R = mnav_fol::fol_tick(M, I, st, Fd, costs, C, W.pos, W.dir, W.up, W.face, list);
    if (how_hist) ++how_hist[R.how];
    smp_after_tick(W, R, P, Q, c, GPtr<const float>(potential), goal_pos, goal_dir);
  }
}
#endif

// What the last call tells of itself (mnav_sample_stats): the rollout's counters over the rows, and the pick's.
struct Stats {
  mnav_rol::Stats rol; uint32_t lethal_rows = 0, feasible_rows = 0, robots_without_pick = 0; float ms_expand = 0.f, ms_pick = 0.f;
};
enum : int { kCntLethal = 0, kCntFeasible = 1, kCntNoPick = 2, kPickCounters = 4 };

#if defined(__HIPCC__)

// what the policy and the kernels around the ticks see beside the rollout's Batch (whose pos, dir, face, slot, seed_face and
// state are per ROW, its up, goal_pos, goal_dir per ROBOT)
struct Sample {
  uint32_t K; Rule Q; const double* table; const float* const* pots;  // pots: the resident potential of every slot a robot uses
  float* pot; uint8_t* lethal; double* cmd0;
};

// the rollout's tick policy over candidate rows: row i is robot i / K under candidate i % K
struct SampleTick : mnav_rol::Tick {
  Sample X;

  __device__ __forceinline__ SampleTick(const mnav_rol::Batch& B, const Params& P_, uint32_t tick, const Sample& X_) : mnav_rol::Tick(B, P_, tick, kNone), X(X_) {}
  __device__ __forceinline__ Row load(uint32_t i, uint32_t f, W3 p) const
  {
    Row W;
    W.pos = p; W.dir = mnav::w3_load(dir + 3 * (size_t)i); W.up = mnav::w3_load(up + 3 * (size_t)(i / X.K));
    W.face = f; W.status = status[i]; W.ticks = ticks[i]; W.travel = travel[i]; W.cost_integral = cost_integral[i];
    W.min_goal_dist = min_goal_dist[i];
    W.pot = X.pot[i]; W.lethal = X.lethal[i]; W.cmd0[0] = 0.0; W.cmd0[1] = 0.0;   // (cmd0 is written by a row's first tick only)
    return W;
  }
  __device__ __forceinline__ int finish(uint32_t i, Row& W, const mnav_fol::Result& R) const
  {
    const uint32_t r = i / X.K, k = i - r * X.K;
    const W3 zero = mnav::w3(0, 0, 0);
    smp_after_tick(W, R, P, X.Q, smp_cand(GPtr<const double>(X.table), k), GPtr<const float>(X.pots[slot[i]]),
                   P.have_goal ? mnav::w3_load(goal_pos + 3 * (size_t)r) : zero, P.have_goal ? mnav::w3_load(goal_dir + 3 * (size_t)r) : zero);
    pos[3 * (size_t)i] = W.pos.x; pos[3 * (size_t)i + 1] = W.pos.y; pos[3 * (size_t)i + 2] = W.pos.z;
    dir[3 * (size_t)i] = W.dir.x; dir[3 * (size_t)i + 1] = W.dir.y; dir[3 * (size_t)i + 2] = W.dir.z;
    face[i] = W.face; status[i] = W.status; ticks[i] = W.ticks; travel[i] = W.travel; cost_integral[i] = W.cost_integral;
    min_goal_dist[i] = W.min_goal_dist;
    X.pot[i] = W.pot; X.lethal[i] = (uint8_t)W.lethal;
    if (W.ticks == 1) { X.cmd0[2 * (size_t)i] = W.cmd0[0]; X.cmd0[2 * (size_t)i + 1] = W.cmd0[1]; }
    return W.status;
  }
};

// the n uploaded robots (a copy: the rows are written over the staging they arrived in); seed_face may be null
struct Robots { const float* pos; const float* dir; const uint32_t* face; const uint32_t* slot; const uint32_t* seed_face; };

// one lane per row: the row of robot i / K before its first tick (smp_start)
__global__ __launch_bounds__(256) void k_sample_expand(Robots In, mnav_rol::Batch B, Sample X, uint32_t* slot_rows, uint32_t* seed_face_rows)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= B.n) return;
  const uint32_t r = i / X.K;
  for (int c = 0; c < 3; ++c) { B.pos[3 * (size_t)i + c] = In.pos[3 * (size_t)r + c]; B.dir[3 * (size_t)i + c] = In.dir[3 * (size_t)r + c]; }
  B.face[i] = In.face[r];
  slot_rows[i] = In.slot[r];
  if (In.seed_face) seed_face_rows[i] = In.seed_face[r];
  B.status[i] = kRunning; B.ticks[i] = 0; B.travel[i] = 0.0; B.cost_integral[i] = 0.0; B.min_goal_dist[i] = INFINITY;
  X.pot[i] = INFINITY; X.lethal[i] = 0; X.cmd0[2 * (size_t)i] = 0.0; X.cmd0[2 * (size_t)i + 1] = 0.0;
}

__global__ __launch_bounds__(mnav_fol::kStayBlock) void k_sample_stay(mnav_rol::Batch B, WalkMesh M, mnav_fol::Config C, Params P, Sample X, uint32_t tick)
{
  mnav_fol::fol_pass_stay(SampleTick(B, P, tick, X), M, C);
}

__global__ __launch_bounds__(64) void k_sample_search(mnav_rol::Batch B, WalkMesh M, mnav_fol::Config C, Params P, Sample X, uint32_t tick)
{
  __shared__ uint32_t list[mnav::kWalkScratchWords];
  mnav_fol::fol_pass_search(SampleTick(B, P, tick, X), M, C, list);
}

__global__ __launch_bounds__(mnav_loc::kLocBlock) void k_sample_global(mnav_rol::Batch B, WalkMesh M, mnav_fol::Config C, Params P, Sample X, mnav_loc::Index I,
                                                                      uint32_t tick)
{
  __shared__ uint32_t s_node[mnav_loc::kStack * mnav_loc::kLocBlock];
  __shared__ float s_bound[mnav_loc::kStack * mnav_loc::kLocBlock];
  const SampleTick T(B, P, tick, X);
  mnav_fol::fol_pass_global(T, M, C, I, T.cnt[1] < T.n ? T.cnt[1] : T.n, s_node, s_bound);
}

// one lane per row: J, and the lethal and feasible rows of the call (one integer atomic per wave and counter)
__global__ __launch_bounds__(256) void k_sample_score(uint32_t rows, const int32_t* status, const uint32_t* ticks, const double* cost_integral, const float* pot,
                                                      const uint8_t* lethal, Weights G, double* score, uint32_t* cnt)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t ic = i < rows ? i : rows - 1;
  const double J = smp_score(pot[ic], cost_integral[ic], ticks[ic], G);
  const uint32_t le = lethal[ic];
  const bool live = i < rows;
  if (live) score[i] = J;
  const unsigned long long bl = __ballot(live && le != 0), bf = __ballot(live && smp_feasible(status[ic], le, J));
  if ((threadIdx.x & 63u) == 0) {
    if (bl) atomicAdd(&cnt[kCntLethal], (uint32_t)__popcll(bl));
    if (bf) atomicAdd(&cnt[kCntFeasible], (uint32_t)__popcll(bf));
  }
}

// one wave per robot, lanes strided over its K rows, then the (J, k) minimum and the count over the 64 lanes
__global__ __launch_bounds__(kPickBlock) void k_sample_pick(uint32_t n, uint32_t K, const int32_t* status, const uint8_t* lethal, const double* score, const double* cmd0,
                                                           uint32_t* best_k, double* best_score, double* best_cmd, uint32_t* n_feasible, uint32_t* cnt)
{
  const uint32_t lane = threadIdx.x & 63u, r = blockIdx.x * (kPickBlock / 64) + (threadIdx.x >> 6);
  if (r >= n) return;                                                 // (wave-uniform)
  const size_t row0 = (size_t)r * K;
  double J = INFINITY; uint32_t k = kNone, count = 0;
  for (uint32_t j = lane; j < K; j += 64u) {
    const double Jj = score[row0 + j];
    if (!smp_feasible(status[row0 + j], lethal[row0 + j], Jj)) continue;
    ++count;
    if (smp_better(J, k, Jj, j)) { J = Jj; k = j; }
  }
  for (int off = 32; off; off >>= 1) {
    const double Jo = __shfl_xor(J, off); const uint32_t ko = (uint32_t)__shfl_xor((int)k, off);
    count += (uint32_t)__shfl_xor((int)count, off);
    if (smp_better(J, k, Jo, ko)) { J = Jo; k = ko; }
  }
  if (lane) return;
  best_k[r] = k; best_score[r] = J; n_feasible[r] = count;
  const size_t kc = k != kNone ? row0 + k : row0;                    // (a clamped row: loaded outside the branch)
  const double c0 = cmd0[2 * kc], c1 = cmd0[2 * kc + 1];
  best_cmd[2 * (size_t)r] = k != kNone ? c0 : 0.0; best_cmd[2 * (size_t)r + 1] = k != kNone ? c1 : 0.0;
  if (k == kNone) atomicAdd(&cnt[kCntNoPick], 1u);
}

// what a sampled rollout keeps on the device beside the staging (the rows' pos, dir, face, slot, seed face and the work
// lists) and the rollout's buffers (the rows' status, ticks, travel, cost integral, smallest goal distance; goals; counter rows)
struct Dev {
  mnav::DevBuf<float> in_pos, in_dir, pot; mnav::DevBuf<uint32_t> in_face, in_slot, in_seed, best_k, n_feasible, cnt; mnav::DevBuf<uint8_t> lethal;
  mnav::DevBuf<double> cmd0, score, table, best_score, best_cmd; mnav::DevBuf<const float*> pots;
  size_t cap = 0, rows_cap = 0, table_cap = 0, slots_cap = 0;
  mnav::Event ev[4]; bool have_ev = false;
};

#endif  // __HIPCC__

}  // namespace mnav_smp
