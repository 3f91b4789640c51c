// mnav_fleet_yield.h -- fleet rollouts in which robots yield (mnav_fleet_rollout_yield): mnav_fleet_rollout.h's check with a
// right-of-way rule evaluated inside its pair pass, whose result keeps a robot from ticking until the next check.  Three
// additions to mnav_fleet_rollout.h, over its grid walk (sep_near) and its host check loop (sep_check_host_each):
//
//   * the rule (include/mnav.h has it in full), in MNAV_HD pieces that device, host mirror and tests share: yld_mover (RUNNING
//     and departed), yld_ahead (partner j lies inside the cone of half angle acos(c) about robot i's heading: dot > 0 &&
//     dot * dot >= c2 * d2, float32, every operation rounded on its own, d2 the pair's sep_d2), yld_before (the lexicographic
//     order of (priority, index)), yld_yields (the decision for one partner) and the fold of a robot's blockers: they go
//     through sep_meet into a Best of their own (smallest d2, ties to the smaller index), and yld_close folds that Best into
//     the robot's YRow.  Compares, counts and minima only, and nothing reads the flags of the check before: one check is a
//     function of the state after its tick, so no order of visits and no earlier check can change a bit.
//
//   * YieldTick, a tick policy derived from FleetTick whose first() also asks hold[i] == 0 and whose idle() counts the ticks
//     a RUNNING, departed robot stood held (pass A calls idle exactly once per robot without a tick).  A held robot is a
//     robot without a tick, like a waiting one.  k_yield_rollout_stay / _search / _global are the unchanged pass bodies of
//     mnav_follow.h over it.  FleetTick's start ticks are never null: the driver supplies zeros.
//
//   * k_yld_pair, the pair pass of a check with the rule.  It visits what k_sep_pair visits (sep_near: every near partner
//     handed to a callable) and folds the same partners into the same separation Row, so the separation outputs are
//     k_sep_pair's bit for bit.  For a near partner only -- the 16-byte records stay as they are -- and among those only for
//     one that is ahead and could still become the blocker, it gathers the partner's status, start tick, heading and
//     priority by id from the resident rows.  It writes hold[i] for every robot (0 for one that is not present, not a mover
//     or yields to nobody), the YRow of a held robot, and adds the held robots of a wave as one integer add to the check's
//     yield row.  A check the guard skips clears hold: with no information nobody is held.
//
// The host mirror yld_check_host runs the same pieces serially, inside sep_check_host's own loop; yld_fold makes a call's
// statistics (YldStats) of the check rows on the host.
#pragma once
#include "mnav_fleet_rollout.h"

namespace mnav_frol {

constexpr int kYldCheckWords = 1;                                     // a check's yield row: robots held
enum : int { kYchkHeld = 0 };

// what a robot knows of its holds after the checks of a call (held_ticks is the tick policy's: idle counts it)
struct YRow { uint32_t hold_checks, first_hold_tick, first_hold_robot; };

// c = (float)ahead_cos; the rule compares squares
MNAV_HD bool yld_cos_ok(float c) { return sep_finite(c) && c >= 0.f && c < 1.f; }

// robot i has a controller tick of its own at call tick `tick` unless something holds it: RUNNING and departed
MNAV_HD bool yld_mover(int32_t status, bool waiting) { return status == mnav_rol::kRunning && !waiting; }

// A(i, j): j is ahead of i.  d2: the pair's sep_d2.  A NaN anywhere compares false; coincident robots give dot == 0
MNAV_HD bool yld_ahead(W3 pi, W3 di, W3 pj, float d2, float c2)
{
  const float ex = pj.x - pi.x, ey = pj.y - pi.y, ez = pj.z - pi.z;
  const float xx = di.x * ex, yy = di.y * ey, zz = di.z * ez;
  const float xy = xx + yy;
  const float dot = xy + zz;
  const float lhs = dot * dot, rhs = c2 * d2;
  return dot > 0.f && lhs >= rhs;
}
// before(j, i): j has right of way over i
MNAV_HD bool yld_before(uint32_t prio_j, uint32_t j, uint32_t prio_i, uint32_t i) { return prio_j < prio_i || (prio_j == prio_i && j < i); }
// a present mover i yields to its partner j: j is ahead, and j does not move, or does not face i, or has right of way
MNAV_HD bool yld_yields(bool ahead_ij, bool mover_j, bool ahead_ji, bool before_ji) { return ahead_ij && (!mover_j || !ahead_ji || before_ji); }

MNAV_HD YRow yld_row_start() { YRow R; R.hold_checks = 0; R.first_hold_tick = kNone; R.first_hold_robot = kNone; return R; }
// blockers: the yielded-to partners of one robot at one check, met through sep_meet
MNAV_HD void yld_close(YRow& R, const Best& blockers, uint32_t tick)
{
  if (!blockers.partners) return;
  R.hold_checks += 1;
  if (R.first_hold_tick == kNone) { R.first_hold_tick = tick; R.first_hold_robot = blockers.id; }
}

// the per-robot yield outputs as arrays (device or host)
struct YRows { uint32_t* hold_checks; uint32_t* held_ticks; uint32_t* first_hold_tick; uint32_t* first_hold_robot; };
MNAV_HD YRow yld_row_load(const YRows& A, uint32_t i) { YRow R; R.hold_checks = A.hold_checks[i]; R.first_hold_tick = A.first_hold_tick[i]; R.first_hold_robot = A.first_hold_robot[i]; return R; }
MNAV_HD void yld_row_store(const YRows& A, uint32_t i, const YRow& R) { A.hold_checks[i] = R.hold_checks; A.first_hold_tick[i] = R.first_hold_tick; A.first_hold_robot[i] = R.first_hold_robot; }

// the resident rows a decision gathers from, by robot id; start_tick and priority may be null (all 0)
struct YGather { const float* pos; const float* dir; const int32_t* status; const uint32_t* start_tick; const uint32_t* priority; float c2; };

// One present robot i at the check after call tick `tick`: its partners into `partners` (what k_sep_pair folds), those it
// yields to into `blockers` -- its d2 / id are the blocker's, its count is only zero or not (see below).  Only a mover asks
// anything of a partner's row.
template <class Keys>
MNAV_HD void yld_robot(const Grid& G, const Keys* keys, uint32_t mask, const uint32_t* cnt, const uint32_t* start, const float* rec, const YGather& Y, uint32_t i,
                       uint32_t tick, Best& partners, Best& blockers)
{
  const W3 p = mnav::w3_load(Y.pos + 3 * (size_t)i);
  const bool mover = yld_mover(Y.status[i], Y.start_tick && frol_waits(tick, Y.start_tick[i]));
  const W3 di = mover ? mnav::w3_load(Y.dir + 3 * (size_t)i) : mnav::w3(0, 0, 0);
  const uint32_t prio_i = Y.priority ? Y.priority[i] : 0u;
  sep_near(G, keys, mask, cnt, start, rec, i, p, [&](uint32_t j, float d2, W3 pj) {
    sep_meet(partners, d2, j);
    if (!mover) return;
    // a robot that is held already asks only partners that could become its blocker (nearer, or as near with a smaller
    // index): the flag and the blocker are all that leaves this function, `blockers.partners` is read as zero / non-zero
    if (blockers.partners && !(d2 < blockers.d2 || (d2 == blockers.d2 && j < blockers.id))) return;
    if (!yld_ahead(p, di, pj, d2, Y.c2)) return;
    const bool mover_j = yld_mover(Y.status[j], Y.start_tick && frol_waits(tick, Y.start_tick[j]));
    bool gives_way = true;
    if (mover_j) {
      const bool ahead_ji = yld_ahead(pj, mnav::w3_load(Y.dir + 3 * (size_t)j), p, d2, Y.c2);
      gives_way = yld_yields(true, true, ahead_ji, yld_before(Y.priority ? Y.priority[j] : 0u, j, prio_i, i));
    }
    if (gives_way) sep_meet(blockers, d2, j);
  });
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The host mirror of one check with the rule: sep_check_host's `rows` and `chk` out of the same loop, and hold (n bytes,
// every one written), yrows and ychk (kYldCheckWords).  Returns false when the guard skipped the pair pass: hold is all 0.
inline bool yld_check_host(uint32_t n, const float* pos, const float* dir, const int32_t* status, const uint32_t* start_tick, const uint32_t* priority, uint32_t tick,
                           uint32_t flags, const Grid& G, float c2, uint32_t table_size, uint64_t max_tests, const Rows& rows, const YRows& yrows, uint8_t* hold,
                           uint64_t* chk, uint32_t* ychk)
{
  for (uint32_t i = 0; i < n; ++i) hold[i] = 0;
  ychk[kYchkHeld] = 0;
  const YGather Y{ pos, dir, status, start_tick, priority, c2 };
  return sep_check_host_each(n, pos, status, start_tick, tick, flags, G, table_size, max_tests, rows, chk, [&](const HostGrid& H, uint32_t i, Best& b) {
    Best blockers = sep_best_start();
    yld_robot(G, H.keys.data(), H.mask, H.cnt.data(), H.start.data(), H.rec.data(), Y, i, tick, b, blockers);
    if (!blockers.partners) return;
    YRow R = yld_row_load(yrows, i);
    yld_close(R, blockers, tick);
    yld_row_store(yrows, i, R);
    hold[i] = 1; ychk[kYchkHeld] += 1;
  });
}
#endif

// What a call tells of its holds afterwards (mnav_fleet_yield_stats); `= {}` is the reset.  A record of its own: the other
// entry points leave it alone, and mnav_fleet_rollout_yield leaves theirs.
struct YldStats {
  uint32_t robots_held = 0, max_held = 0, max_held_tick = kNone, held_last = 0, checks_run = 0, checks_skipped = 0, first_skipped_tick = kNone;
  uint64_t held_ticks = 0;
  float ms_pair = 0.f, ms_separation = 0.f, ms_kernels = 0.f, ms_total = 0.f;
};

// The separation rows (for their skipped flags) and the yield rows of the `checks` checks a call of n robots ran, two of the
// robots' columns and the flags as they stand at the end, folded into a reset S, on the host.  A skipped check held nobody
// and is no candidate for the maximum; the first check run with the most robots held gives max_held_tick.  The checks run
// and skipped and the first skipped one's tick are counted as sep_fold counts them.
inline void yld_fold(const uint64_t* chk, const uint32_t* ychk, uint32_t checks, uint32_t check_stride, uint32_t n, const uint32_t* hold_checks,
                     const uint32_t* held_ticks, const uint8_t* hold, YldStats& S)
{
  for (uint32_t c = 0; c < checks; ++c) {
    if (chk[(size_t)kCheckWords * c + kChkSkipped]) { if (!S.checks_skipped++) S.first_skipped_tick = (c + 1) * check_stride; continue; }
    S.checks_run += 1;
    const uint32_t held = ychk[(size_t)kYldCheckWords * c + kYchkHeld];
    if (S.max_held_tick == kNone || held > S.max_held) { S.max_held = held; S.max_held_tick = (c + 1) * check_stride; }
  }
  for (uint32_t i = 0; i < n; ++i) {
    if (hold_checks[i]) S.robots_held += 1;
    S.held_ticks += held_ticks[i];
    if (hold[i]) S.held_last += 1;
  }
}

#if defined(__HIPCC__)

// The fleet's tick with holds: robot i has no tick while hold[i] is set.  idle() sees every robot without a tick once, in
// pass A: the one that is RUNNING and has departed is held.
struct YieldTick : FleetTick {
  const uint8_t* hold; uint32_t* held_ticks;

  __device__ __forceinline__ YieldTick(const mnav_rol::Batch& B, const mnav_rol::Params& P_, uint32_t tick_, uint32_t trace_row_, const uint32_t* start_tick_,
                                       const uint8_t* hold_, uint32_t* held_ticks_)
      : FleetTick(B, P_, tick_, trace_row_, start_tick_), hold(hold_), held_ticks(held_ticks_) {}
  __device__ __forceinline__ bool first(uint32_t ic, uint32_t& f, W3& p) const
  {
    const bool departed = FleetTick::first(ic, f, p);
    return departed && hold[ic] == 0;
  }
  __device__ __forceinline__ void idle(uint32_t i, W3 p) const
  {
    trace_at(i, p);
    if (yld_mover(status[i], frol_waits(tick + 1, start_tick[i]))) held_ticks[i] += 1;   // (first() was false: it is held)
  }
};

__global__ __launch_bounds__(mnav_fol::kStayBlock) void k_yield_rollout_stay(mnav_rol::Batch B, mnav::WalkMesh M, mnav_fol::Config C, mnav_rol::Params P, uint32_t tick,
                                                                              uint32_t trace_row, const uint32_t* start_tick, const uint8_t* hold, uint32_t* held_ticks)
{
  mnav_fol::fol_pass_stay(YieldTick(B, P, tick, trace_row, start_tick, hold, held_ticks), M, C);
}

__global__ __launch_bounds__(64) void k_yield_rollout_search(mnav_rol::Batch B, mnav::WalkMesh M, mnav_fol::Config C, mnav_rol::Params P, uint32_t tick,
                                                             uint32_t trace_row, const uint32_t* start_tick, const uint8_t* hold, uint32_t* held_ticks)
{
  __shared__ uint32_t list[mnav::kWalkScratchWords];
  mnav_fol::fol_pass_search(YieldTick(B, P, tick, trace_row, start_tick, hold, held_ticks), M, C, list);
}

__global__ __launch_bounds__(mnav_loc::kLocBlock) void k_yield_rollout_global(mnav_rol::Batch B, mnav::WalkMesh M, mnav_fol::Config C, mnav_rol::Params P,
                                                                              mnav_loc::Index I, uint32_t tick, uint32_t trace_row, const uint32_t* start_tick,
                                                                              const uint8_t* hold, uint32_t* held_ticks)
{
  __shared__ uint32_t s_node[mnav_loc::kStack * mnav_loc::kLocBlock];
  __shared__ float s_bound[mnav_loc::kStack * mnav_loc::kLocBlock];
  const YieldTick T(B, P, tick, trace_row, start_tick, hold, held_ticks);
  mnav_fol::fol_pass_global(T, M, C, I, T.cnt[1] < T.n ? T.cnt[1] : T.n, s_node, s_bound);
}

// what the pair pass with the rule sees beside Sep: the headings, the priorities (may be null), the flags it writes, the
// call's yield check rows and the robots' yield rows
struct Yld { float c2; const float* dir; const uint32_t* priority; uint8_t* hold; uint32_t* ychk; YRows rows; };

__device__ __forceinline__ uint32_t yld_wave_sum(uint32_t v)
{
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
  return v;
}

// k_sep_pair with the rule.  Only robot i writes row i, yield row i and hold[i]; every i < n gets its hold written.
__global__ __launch_bounds__(kSepBlock) void k_yld_pair(Sep S, Yld Y, uint32_t check, uint32_t tick)
{
  unsigned long long* row = S.chk + (size_t)kCheckWords * check;
  const uint32_t i = blockIdx.x * kSepBlock + threadIdx.x;
  if (row[kChkTests] > S.max_tests) {                                 // (final: k_sep_fill has ended; uniform over the grid)
    if (blockIdx.x == 0 && threadIdx.x == 0) row[kChkSkipped] = 1;
    if (i < S.n) Y.hold[i] = 0;                                       // with no information nobody is held
    return;
  }
  unsigned long long partners = 0;
  uint32_t held = 0;
  if (i < S.n) {
    if (S.slot_of[i] != kNone) {
      Best b = sep_best_start(), blockers = sep_best_start();
      const YGather Q{ S.pos, Y.dir, S.status, S.start_tick, Y.priority, Y.c2 };
      yld_robot(S.G, S.keys, S.mask, S.cnt, S.start, S.rec, Q, i, tick, b, blockers);
      if (b.partners) {
        Row R = sep_row_load(S.rows, i);
        sep_close(R, b, tick);
        sep_row_store(S.rows, i, R);
      }
      if (blockers.partners) {
        YRow H = yld_row_load(Y.rows, i);
        yld_close(H, blockers, tick);
        yld_row_store(Y.rows, i, H);
        held = 1;
      }
      partners = b.partners;
    }
    Y.hold[i] = (uint8_t)held;
  }
  partners = sep_wave_sum(partners);
  held = yld_wave_sum(held);
  if ((threadIdx.x & 63u) == 0) {
    if (partners) atomicAdd(&row[kChkOrdered], partners);
    if (held) atomicAdd(&Y.ychk[(size_t)kYldCheckWords * check + kYchkHeld], held);
  }
}

// what a yielding fleet rollout adds on the device to mnav_frol::State (grown on demand, kept between calls): the flags, the
// priorities, the robots' yield rows, the yield check rows and the event pairs that time the pair passes of a block
struct YldState {
  mnav::DevBuf<uint8_t> hold; mnav::DevBuf<uint32_t> priority, hold_checks, held_ticks, first_hold_tick, first_hold_robot, ychk;
  size_t cap = 0, chk_cap = 0;
  mnav::Event ev[2 * mnav_rol::kBlockTicks]; bool have_ev = false;
};

#endif  // __HIPCC__

}  // namespace mnav_frol
