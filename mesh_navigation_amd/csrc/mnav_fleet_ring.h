// mnav_fleet_ring.h -- wait-for analysis of a yielding fleet rollout (mnav_fleet_rollout_rings): why a held robot is held, and
// the release of rings.  Over mnav_fleet_yield.h: the same tick kernels, the same rule, the same flags.  "Held robot -> its
// blocker" is a functional graph, w(i) = blocker[i] for a held robot and i for one that is not; its fixed points are the robots
// that are not held (ROOTS), its other cycles are RINGS (include/mnav.h has the terms in full).  Per check, after the pair pass:
//
//   k_ring_pair    k_yld_pair once more -- the same yld_robot, the same row updates, the same hold, the same wave-reduced add
//                  into the yield check row -- which also keeps blocker[i] (kNone for a robot that is not held) and starts the
//                  doubling: jump0[i] = w(i), key0[i] = (priority << 32) | i, mark[i] = 0
//   k_ring_double  K = ceil(log2 max(n, 2)) launches over ping-pong buffers: jump'[i] = jump[jump[i]], key'[i] = min(key[i],
//                  key[jump[i]]).  After k rounds jump is w applied 2^k times and key the smallest key of the 2^k nodes from i on.
//                  With 2^k >= H, the robots held (final in the yield check row since the pair pass ended), a chain has left its
//                  tail: jump[i] is the root or lies on the ring, and a ring node's key is its leader's.  A round with 2^k >= H
//                  already returns at once when the early exit is on (option ring_early_exit, off by default: measured, it
//                  does not pay; ring_rounds says how many rounds ran, hence which buffer holds the result); root, leader and
//                  marks are the same for every k with 2^k >= H.
//   k_ring_close   a held lane i: r = jump[i]; r not held: QUEUED or PARKED by yld_mover of r, anchor r.  r held: anchor = the
//                  low word of key[r], mark[r] = 1 (a scatter of equal bytes), class RING_TAIL for now.  A tail holds fewer than
//                  H <= 2^k robots, so no tail node is the image of 2^k steps, and every ring node is: w^(2^k) permutes a ring.
//   k_ring_rows    mark[i] makes a RING_TAIL a RING_MEMBER; the member that is its own anchor is the leader, counts the ring
//                  and, with MNAV_RING_RELEASE, clears its own hold; the robot's ring row; wave-reduced integer adds into the
//                  check's ring row.
//
// "Held" is read from blocker (!= kNone), never from hold, which k_ring_rows changes.  Integers only, no kernel waits for
// another workgroup, every gather is unconditional at an index below n.  The host mirror ring_check_host runs the same
// MNAV_HD pieces serially; ring_fold makes a call's statistics (RingStats) of the check rows.
#pragma once
#include "mnav_fleet_yield.h"

namespace mnav_frol {

constexpr uint32_t kRingRelease = 1u, kRingKnownFlags = 1u;          // MNAV_RING_*, include/mnav.h
constexpr uint8_t kWaitFree = 0, kWaitQueued = 1, kWaitParked = 2, kWaitRingTail = 3, kWaitRingMember = 4;   // MNAV_WAIT_*
constexpr int kRingCheckWords = 6;                                    // a check's ring row
enum : int { kRchkQueued = 0, kRchkParked = 1, kRchkTails = 2, kRchkMembers = 3, kRchkRings = 4, kRchkReleased = 5 };

// what a robot knows of its waits after the checks of a call
struct RRow { uint32_t ring_checks, first_ring_tick, parked_checks, released_checks; };
// the per-robot ring outputs as arrays (device or host); wait_class and anchor are the last check's
struct RRows { uint32_t* ring_checks; uint32_t* first_ring_tick; uint32_t* parked_checks; uint32_t* released_checks; uint8_t* wait_class; uint32_t* anchor; };

// the order of yld_before as one integer
MNAV_HD uint64_t ring_key(uint32_t priority, uint32_t i) { return ((uint64_t)priority << 32) | i; }
// the launches per check for n robots: the smallest K with 2^K >= max(n, 2)
MNAV_HD uint32_t ring_launches(uint32_t n) { uint32_t k = 1; while (k < 32 && (1ull << k) < n) ++k; return k; }
// of `launched` rounds over a check that holds `held` robots, how many did not return at once: all without the early exit, else
// the smallest k with 2^k >= held (0 for held <= 1).  launched >= that k, as held <= n.  The result lies in buffer (rounds & 1).
MNAV_HD uint32_t ring_rounds(uint32_t held, uint32_t launched, bool early)
{
  if (!early) return launched;
  uint32_t k = 0;
  while (k < launched && (1ull << k) < held) ++k;
  return k;
}
// one round for robot i (jump[i] < n)
template <class Key>
MNAV_HD void ring_step(const uint32_t* jump, const Key* key, uint32_t i, uint32_t& jump_out, uint64_t& key_out)
{
  const uint32_t j = jump[i];
  const uint64_t a = (uint64_t)key[i], b = (uint64_t)key[j];
  jump_out = jump[j];
  key_out = a < b ? a : b;
}
// a held robot whose chain reaches r: not yet told apart, a ring's member is a RING_TAIL
MNAV_HD void ring_classify(bool held_r, bool mover_r, uint32_t r, uint64_t key_r, uint8_t& cls, uint32_t& anchor)
{
  if (held_r) { cls = kWaitRingTail; anchor = (uint32_t)key_r; }
  else { cls = mover_r ? kWaitQueued : kWaitParked; anchor = r; }
}
MNAV_HD void ring_close(RRow& R, uint8_t cls, bool released, uint32_t tick)
{
  if (cls == kWaitRingMember) { R.ring_checks += 1; if (R.first_ring_tick == kNone) R.first_ring_tick = tick; }
  if (cls == kWaitParked) R.parked_checks += 1;
  if (released) R.released_checks += 1;
}
MNAV_HD RRow ring_row_load(const RRows& A, uint32_t i) { RRow R; R.ring_checks = A.ring_checks[i]; R.first_ring_tick = A.first_ring_tick[i]; R.parked_checks = A.parked_checks[i]; R.released_checks = A.released_checks[i]; return R; }
MNAV_HD void ring_row_store(const RRows& A, uint32_t i, const RRow& R) { A.ring_checks[i] = R.ring_checks; A.first_ring_tick[i] = R.first_ring_tick; A.parked_checks[i] = R.parked_checks; A.released_checks[i] = R.released_checks; }

#if !defined(__HIP_DEVICE_COMPILE__)
// The host mirror of one check with the rule and the analysis: yld_check_host's outputs out of the same loop (hold as it
// stands after the release), the ring rows, wait_class and anchor of every robot and rchk (kRingCheckWords).  launched: the
// rounds of the doubling, at least ring_launches of the robots held.  Returns false when the guard skipped the pair pass:
// hold is all 0, every class FREE, every anchor kNone, rchk all 0.
inline bool ring_check_host(uint32_t n, const float* pos, const float* dir, const int32_t* status, const uint32_t* start_tick, const uint32_t* priority, uint32_t tick,
                            uint32_t flags, const Grid& G, float c2, uint32_t table_size, uint64_t max_tests, const Rows& rows, const YRows& yrows, uint8_t* hold,
                            uint64_t* chk, uint32_t* ychk, uint32_t ring_flags, uint32_t launched, bool early, const RRows& rrows, uint32_t* rchk)
{
  std::vector<uint32_t> blocker(n, kNone), jump[2] = { std::vector<uint32_t>(n), std::vector<uint32_t>(n) };
  std::vector<uint64_t> key[2] = { std::vector<uint64_t>(n), std::vector<uint64_t>(n) };
  std::vector<uint8_t> mark(n, 0);
  for (uint32_t i = 0; i < n; ++i) { hold[i] = 0; rrows.wait_class[i] = kWaitFree; rrows.anchor[i] = kNone; }
  for (int k = 0; k < kRingCheckWords; ++k) rchk[k] = 0;
  ychk[kYchkHeld] = 0;
  const YGather Y{ pos, dir, status, start_tick, priority, c2 };
  const bool ran = sep_check_host_each(n, pos, status, start_tick, tick, flags, G, table_size, max_tests, rows, chk, [&](const HostGrid& H, uint32_t i, Best& b) {
    Best blockers = sep_best_start();
    yld_robot(G, H.keys.data(), H.mask, H.cnt.data(), H.start.data(), H.rec.data(), Y, i, tick, b, blockers);
    if (!blockers.partners) return;
    YRow R = yld_row_load(yrows, i);
    yld_close(R, blockers, tick);
    yld_row_store(yrows, i, R);
    hold[i] = 1; ychk[kYchkHeld] += 1; blocker[i] = blockers.id;
  });
  if (!ran) return false;
  for (uint32_t i = 0; i < n; ++i) { jump[0][i] = blocker[i] != kNone ? blocker[i] : i; key[0][i] = ring_key(priority ? priority[i] : 0u, i); }
  const uint32_t rounds = ring_rounds(ychk[kYchkHeld], launched, early);
  for (uint32_t k = 0; k < rounds; ++k)
    for (uint32_t i = 0; i < n; ++i) ring_step(jump[k & 1].data(), key[k & 1].data(), i, jump[~k & 1][i], key[~k & 1][i]);
  const std::vector<uint32_t>& J = jump[rounds & 1];
  const std::vector<uint64_t>& K = key[rounds & 1];
  for (uint32_t i = 0; i < n; ++i) {
    if (blocker[i] == kNone) continue;
    const uint32_t r = J[i];
    const bool held_r = blocker[r] != kNone;
    ring_classify(held_r, yld_mover(status[r], start_tick && frol_waits(tick, start_tick[r])), r, K[r], rrows.wait_class[i], rrows.anchor[i]);
    if (held_r) mark[r] = 1;
  }
  for (uint32_t i = 0; i < n; ++i) {
    uint8_t cls = rrows.wait_class[i];
    if (cls == kWaitRingTail && mark[i]) cls = kWaitRingMember;
    const bool leader = cls == kWaitRingMember && rrows.anchor[i] == i, released = leader && (ring_flags & kRingRelease);
    if (released) hold[i] = 0;
    rrows.wait_class[i] = cls;
    RRow R = ring_row_load(rrows, i);
    ring_close(R, cls, released, tick);
    ring_row_store(rrows, i, R);
    rchk[kRchkQueued] += cls == kWaitQueued; rchk[kRchkParked] += cls == kWaitParked; rchk[kRchkTails] += cls == kWaitRingTail;
    rchk[kRchkMembers] += cls == kWaitRingMember; rchk[kRchkRings] += leader; rchk[kRchkReleased] += released;
  }
  return true;
}
#endif

// What a call tells of its waits afterwards (mnav_fleet_ring_stats); `= {}` is the reset.  A record of its own.
struct RingStats {
  uint32_t robots_ring = 0, max_rings = 0, max_rings_tick = kNone, members_last = 0, tails_last = 0, parked_last = 0, queued_last = 0, rings_last = 0, checks_run = 0,
           checks_skipped = 0, first_skipped_tick = kNone;
  uint64_t rings = 0, releases = 0;
  float ms_ring = 0.f, ms_separation = 0.f, ms_kernels = 0.f, ms_total = 0.f;
};

// The separation rows (for their skipped flags) and the ring rows of the `checks` checks a call of n robots ran and one of the
// robots' columns, folded into a reset S, on the host.  A skipped check counted nothing and is no candidate for the maximum;
// the first check run with the most rings gives max_rings_tick.  The *_last values are the row of the call's last check (all 0
// when the guard skipped it or no check ran).
inline void ring_fold(const uint64_t* chk, const uint32_t* rchk, uint32_t checks, uint32_t check_stride, uint32_t n, const uint32_t* ring_checks, RingStats& S)
{
  for (uint32_t c = 0; c < checks; ++c) {
    if (chk[(size_t)kCheckWords * c + kChkSkipped]) { if (!S.checks_skipped++) S.first_skipped_tick = (c + 1) * check_stride; continue; }
    S.checks_run += 1;
    const uint32_t* row = rchk + (size_t)kRingCheckWords * c;
    S.rings += row[kRchkRings]; S.releases += row[kRchkReleased];
    if (S.max_rings_tick == kNone || row[kRchkRings] > S.max_rings) { S.max_rings = row[kRchkRings]; S.max_rings_tick = (c + 1) * check_stride; }
  }
  if (checks && !chk[(size_t)kCheckWords * (checks - 1) + kChkSkipped]) {
    const uint32_t* row = rchk + (size_t)kRingCheckWords * (checks - 1);
    S.members_last = row[kRchkMembers]; S.tails_last = row[kRchkTails]; S.parked_last = row[kRchkParked]; S.queued_last = row[kRchkQueued]; S.rings_last = row[kRchkRings];
  }
  for (uint32_t i = 0; i < n; ++i) if (ring_checks[i]) S.robots_ring += 1;
}

#if defined(__HIPCC__)

// what the kernels of the analysis see beside Sep and Yld: the ring flags, whether a covered round returns at once, the
// blockers, the ping-pong buffers of the doubling, the marks, the robots' ring rows and the call's ring check rows
struct Ring {
  uint32_t flags, early, launched;
  uint32_t* blocker; uint32_t* jump[2]; unsigned long long* key[2]; uint8_t* mark; uint32_t* rchk; RRows rows;
};

// k_yld_pair, which also keeps the blocker and starts the doubling.  Only robot i writes its own entries; every i < n gets
// its hold, blocker, jump0, key0 and mark written, also at a check that the guard skips (nobody held: every class FREE).
__global__ __launch_bounds__(kSepBlock) void k_ring_pair(Sep S, Yld Y, Ring Q, uint32_t check, uint32_t tick)
{
  unsigned long long* row = S.chk + (size_t)kCheckWords * check;
  const uint32_t i = blockIdx.x * kSepBlock + threadIdx.x;
  const bool skipped = row[kChkTests] > S.max_tests;                  // (final: k_sep_fill has ended; uniform over the grid)
  if (skipped && blockIdx.x == 0 && threadIdx.x == 0) row[kChkSkipped] = 1;
  unsigned long long partners = 0;
  uint32_t held = 0;
  if (i < S.n) {
    uint32_t blocker = kNone;
    if (!skipped && S.slot_of[i] != kNone) {
      Best b = sep_best_start(), blockers = sep_best_start();
      const YGather G{ S.pos, Y.dir, S.status, S.start_tick, Y.priority, Y.c2 };
      yld_robot(S.G, S.keys, S.mask, S.cnt, S.start, S.rec, G, i, tick, b, blockers);
      if (b.partners) {
        Row R = sep_row_load(S.rows, i);
        sep_close(R, b, tick);
        sep_row_store(S.rows, i, R);
      }
      if (blockers.partners) {
        YRow H = yld_row_load(Y.rows, i);
        yld_close(H, blockers, tick);
        yld_row_store(Y.rows, i, H);
        held = 1; blocker = blockers.id;
      }
      partners = b.partners;
    }
    Y.hold[i] = (uint8_t)held;
    Q.blocker[i] = blocker;
    Q.jump[0][i] = held ? blocker : i;
    Q.key[0][i] = ring_key(Y.priority ? Y.priority[i] : 0u, i);
    Q.mark[i] = 0;
  }
  if (skipped) return;
  partners = sep_wave_sum(partners);
  held = yld_wave_sum(held);
  if ((threadIdx.x & 63u) == 0) {
    if (partners) atomicAdd(&row[kChkOrdered], partners);
    if (held) atomicAdd(&Y.ychk[(size_t)kYldCheckWords * check + kYchkHeld], held);
  }
}

// round k of the doubling: buffer (k & 1) into buffer (~k & 1).  Returns at once when the rounds before cover the robots held.
__global__ __launch_bounds__(kSepBlock) void k_ring_double(Ring Q, uint32_t n, const uint32_t* ychk, uint32_t check, uint32_t k)
{
  const uint32_t held = ychk[(size_t)kYldCheckWords * check + kYchkHeld];   // (final: the pair pass has ended; uniform over the grid)
  if (k >= ring_rounds(held, Q.launched, Q.early != 0)) return;
  const uint32_t i = blockIdx.x * kSepBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t j; uint64_t key;
  ring_step(Q.jump[k & 1], Q.key[k & 1], i, j, key);
  Q.jump[~k & 1][i] = j; Q.key[~k & 1][i] = key;
}

// the provisional class and the anchor of every robot, the marks of the ring nodes
__global__ __launch_bounds__(kSepBlock) void k_ring_close(Sep S, Ring Q, const uint32_t* ychk, uint32_t check, uint32_t tick)
{
  const uint32_t i = blockIdx.x * kSepBlock + threadIdx.x;
  if (i >= S.n) return;
  const uint32_t at = ring_rounds(ychk[(size_t)kYldCheckWords * check + kYchkHeld], Q.launched, Q.early != 0) & 1u;
  const bool held = Q.blocker[i] != kNone;
  uint32_t r = Q.jump[at][i];                                         // (a robot that is not held: itself)
  r = r < S.n ? r : i;
  const bool held_r = Q.blocker[r] != kNone;
  const uint64_t key_r = Q.key[at][r];
  const bool mover_r = yld_mover(S.status[r], S.start_tick && frol_waits(tick, S.start_tick[r]));
  uint8_t cls = kWaitFree; uint32_t anchor = kNone;
  if (held) {
    ring_classify(held_r, mover_r, r, key_r, cls, anchor);
    if (held_r) Q.mark[r] = 1;
  }
  Q.rows.wait_class[i] = cls; Q.rows.anchor[i] = anchor;
}

// the lanes of a wave for which `is` holds, as one integer add (every lane of the wave calls it)
__device__ __forceinline__ void ring_wave_add(uint32_t* at, bool is)
{
  const unsigned long long lanes = __ballot(is);
  if ((threadIdx.x & 63u) == 0 && lanes) atomicAdd(at, (uint32_t)__popcll(lanes));
}

// members from tails, the leaders' release, the robots' ring rows, the check's ring row
__global__ __launch_bounds__(kSepBlock) void k_ring_rows(Ring Q, uint32_t n, uint8_t* hold, uint32_t check, uint32_t tick)
{
  const uint32_t i = blockIdx.x * kSepBlock + threadIdx.x;
  uint8_t cls = kWaitFree;
  bool leader = false, released = false;
  if (i < n) {
    cls = Q.rows.wait_class[i];
    if (cls != kWaitFree) {
      if (cls == kWaitRingTail && Q.mark[i]) { cls = kWaitRingMember; Q.rows.wait_class[i] = cls; }
      leader = cls == kWaitRingMember && Q.rows.anchor[i] == i;
      released = leader && (Q.flags & kRingRelease);
      if (released) hold[i] = 0;
      if (cls == kWaitRingMember || cls == kWaitParked) {
        RRow R = ring_row_load(Q.rows, i);
        ring_close(R, cls, released, tick);
        ring_row_store(Q.rows, i, R);
      }
    }
  }
  uint32_t* row = Q.rchk + (size_t)kRingCheckWords * check;
  ring_wave_add(&row[kRchkQueued], cls == kWaitQueued);
  ring_wave_add(&row[kRchkParked], cls == kWaitParked);
  ring_wave_add(&row[kRchkTails], cls == kWaitRingTail);
  ring_wave_add(&row[kRchkMembers], cls == kWaitRingMember);
  ring_wave_add(&row[kRchkRings], leader);
  ring_wave_add(&row[kRchkReleased], released);
}

// what the analysis adds on the device to YldState (grown on demand, kept between calls): 28 bytes per robot of blockers and
// ping-pong buffers, the marks, the classes, the anchors and ring rows, a ring row per check, and the event pairs that time
// the kernels behind the pair pass
struct RingState {
  mnav::DevBuf<uint32_t> blocker, jump0, jump1, anchor, ring_checks, first_ring_tick, parked_checks, released_checks, rchk;
  mnav::DevBuf<unsigned long long> key0, key1; mnav::DevBuf<uint8_t> mark, wait_class;
  size_t cap = 0, chk_cap = 0;
  mnav::Event ev[2 * mnav_rol::kBlockTicks]; bool have_ev = false;
};

#endif  // __HIPCC__

}  // namespace mnav_frol
