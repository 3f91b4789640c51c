// mnav_fleet_rollout.h -- fleet rollouts (mnav_fleet_rollout): mnav_follow_rollout with a departure tick per robot and a
// separation check between the robots on the device.  Two additions to mnav_rollout.h:
//
//   * FleetTick, a tick policy derived from mnav_rol::Tick whose first() also asks `tick >= start_tick[i]` (device ticks
//     count from 0: frol_waits(tick + 1, start_tick[i]) is false).  A waiting robot is a robot without a tick -- idle()
//     repeats its position in the trace, nothing else of its row is read or written -- so k_fleet_rollout_stay / _search /
//     _global are the three passes of mnav_follow.h once more, and a robot that has departed runs mnav_rollout.h's rule.
//     They run when a call has start ticks; one without runs k_rollout_*, so FleetTick does not test for null.
//
//   * the check.  After all passes of call tick t with t % check_stride == 0 every PRESENT robot (sep_present) learns
//     which other present robots stand within the radius: d2 = (dx*dx + dy*dy) + dz*dz <= r2 in float32 (sep_d2, symmetric
//     in its arguments).  One check folds a robot's partners into a Best (sep_meet: count, smallest d2, ties to the smaller
//     index) and the Best into the robot's Row (sep_close: counts and minima only), so no order of visits can change a bit.
//
// The grid: cells of side h = cell_scale * max(r, 1.8e-18), coordinate c(x) = clamp(floorf(x / h)) to 21 bits, three of them packed
// into a 64-bit key, keys in an open-addressing table of M >= 2 n slots (linear probing, 64-bit compare-and-swap).
// CONSERVATIVENESS (DESIGN.md section 3.20 has the argument in full): robot i searches the cells [c(lo), c(hi)] per axis
// with lo = below(x - reach), hi = above(x + reach), reach = 1.001 r + 1.8e-18 and below / above = the neighbouring float.
// d2 <= r2 implies |fl(xi - xj)| <= reach (sep_grid), hence lo <= xj <= hi as floats, and c() is monotone (a correctly
// rounded division, floorf and a clamp are), so c(lo) <= c(xj) <= c(hi) for every allowed cell_scale.  Where x / h leaves
// the 21 bits the coordinate saturates: far robots share the boundary cells, which costs tests and never a pair.  Before
// saturation ulp(x) <= h / 8, so a range spans at most 5 cells per axis (7 for radii below 1.8e-18).
//
// Device shape, per check, on the context's stream between two ticks (nothing goes to the host):
//   k_sep_clear    the table's keys and counts
//   k_sep_insert   one lane per robot: presence, key, slot (sep_insert), rank = atomicAdd(count[slot], 1)
//   k_sep_sums / k_sep_top / k_sep_starts   exclusive scan of the counts in slot order (tiles of 2048 slots: tile sums, one
//                  workgroup over the tile sums, every tile over its own counts; no kernel waits for another workgroup)
//   k_sep_fill     record (x, y, z, id) at start[slot] + rank; T += the populations of the cells in the robot's range
//                  (sep_tests; uint64, one atomic per wave): the distance tests the pair pass would perform; largest cell
//   k_sep_pair     T > separation_max_tests: the check is SKIPPED (flag in the check's row, read here, no host round trip).
//                  Else one lane per robot streams the records of its range (sep_near); only robot i writes row i; the
//                  near partners of a wave go as one 64-bit add into the check's row.
// The atomics decide a record's place inside its cell and a key's slot in the table; neither is visible in an output.
// One walk, sep_cells, visits a range's cells for sep_tests and sep_near.  The host mirror runs the same MNAV_HD pieces
// serially (HostGrid, sep_check_host_each, sep_check_host); sep_fold makes a call's statistics (SepStats) of its check rows.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "mnav_rollout.h"

namespace mnav_frol {

using mnav::kNone;
using mnav::W3;

constexpr uint32_t kWaitingPresent = 1u, kReachedPresent = 2u, kKnownFlags = 3u;   // MNAV_SEP_*, include/mnav.h
constexpr uint64_t kEmptyKey = ~0ull;                                 // no cell: a key has 63 bits
constexpr int kCellLimit = 1 << 20;                                   // cell coordinates: -2^20 .. 2^20 - 1
constexpr float kDefaultCellScale = 2.0f;
constexpr double kDefaultMaxTests = 4294967296.0;                     // 2^32: provisional
constexpr int kCheckWords = 4;                                        // a check's row: tests T, ordered near pairs, largest cell, skipped
enum : int { kChkTests = 0, kChkOrdered = 1, kChkMaxCell = 2, kChkSkipped = 3 };

struct Grid { float r2, h, reach; };
// what a robot knows of its neighbours after the checks of a call
struct Row { uint32_t near_checks, max_partners, first_near_tick, first_near_robot; float min_sep2; uint32_t min_sep_tick, min_sep_robot; };
// the partners of one robot at one check
struct Best { uint32_t partners; float d2; uint32_t id; };
struct Range { int lo[3], hi[3]; };

MNAV_HD uint32_t sep_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
MNAV_HD float sep_float(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }
MNAV_HD bool sep_finite(float x) { return (sep_bits(x) & 0x7F800000u) != 0x7F800000u; }
// the neighbouring floats of a finite x (an infinity stays: a sum that overflowed is already outside every position)
MNAV_HD float sep_below(float x)
{
  if (!sep_finite(x)) return x;
  if (x == 0.f) return sep_float(0x80000001u);
  const uint32_t u = sep_bits(x);
  return sep_float(x > 0.f ? u - 1 : u + 1);
}
MNAV_HD float sep_above(float x)
{
  if (!sep_finite(x)) return x;
  if (x == 0.f) return sep_float(0x00000001u);
  const uint32_t u = sep_bits(x);
  return sep_float(x > 0.f ? u + 1 : u - 1);
}

// r = (float)radius; kReachFloor = 1.8e-18 >= 2^-59.  reach: two coordinates whose rounded difference dx = fl(a - b) has
// |dx| > 1.0005 r + 2^-60 have fl(dx * dx) > r2, and d2 is at least that square (a rounded sum of non-negative terms is never
// below a term) -- for r >= 2^-62 every number involved is normal and 1.0005^2 exceeds the three roundings (2^-24 each) by
// far; for a smaller r, r2 < 2^-124 while dx * dx > 2^-120.  So a near pair has |dx| <= 1.0005 r + 2^-60, its real
// difference is at most (1 + 2^-24) times that, and reach, rounded twice, is still larger.  h never falls below
// cell_scale * kReachFloor, so that a range stays a few cells wide for any radius (a larger cell costs tests, never a pair).
constexpr float kReachFloor = 1.8e-18f;
MNAV_HD Grid sep_grid(float r, float cell_scale)
{
  Grid G;
  G.r2 = r * r; G.h = cell_scale * (r > kReachFloor ? r : kReachFloor); G.reach = r * 1.001f + kReachFloor;
  return G;
}
MNAV_HD bool sep_grid_ok(const Grid& G) { return sep_finite(G.r2) && G.r2 > 0.f && sep_finite(G.h) && G.h > 0.f && sep_finite(G.reach); }

// monotone in x for x not NaN (h > 0): a correctly rounded division, floorf, a clamp
MNAV_HD int sep_cell(float x, float h)
{
  const float f = floorf(x / h);
  return f <= (float)-kCellLimit ? -kCellLimit : f >= (float)(kCellLimit - 1) ? kCellLimit - 1 : (int)f;
}
MNAV_HD uint64_t sep_key(int cx, int cy, int cz)
{
  return ((uint64_t)(uint32_t)(cx + kCellLimit) << 42) | ((uint64_t)(uint32_t)(cy + kCellLimit) << 21) | (uint64_t)(uint32_t)(cz + kCellLimit);
}
MNAV_HD uint64_t sep_key_of(const Grid& G, W3 p) { return sep_key(sep_cell(p.x, G.h), sep_cell(p.y, G.h), sep_cell(p.z, G.h)); }
MNAV_HD void sep_axis(const Grid& G, float x, int* lo, int* hi)
{
  *lo = sep_cell(sep_below(x - G.reach), G.h);
  *hi = sep_cell(sep_above(x + G.reach), G.h);
}
MNAV_HD Range sep_range(const Grid& G, W3 p)
{
  Range R;
  sep_axis(G, p.x, &R.lo[0], &R.hi[0]); sep_axis(G, p.y, &R.lo[1], &R.hi[1]); sep_axis(G, p.z, &R.lo[2], &R.hi[2]);
  return R;
}
MNAV_HD uint32_t sep_hash(uint64_t k, uint32_t mask)
{
  k ^= k >> 33; k *= 0xFF51AFD7ED558CCDull; k ^= k >> 33; k *= 0xC4CEB9FE1A85EC53ull; k ^= k >> 33;
  return (uint32_t)k & mask;
}

// The table: mask + 1 slots (a power of two, more than the keys it ever holds, so a probe always ends).  cas(slot, key):
// stores key where the slot was empty and returns what it held before.
template <class Cas>
MNAV_HD uint32_t sep_insert(uint32_t mask, uint64_t key, Cas cas)
{
  uint32_t s = sep_hash(key, mask);
  for (uint32_t probes = 0; probes <= mask; ++probes, s = (s + 1) & mask) {
    const uint64_t was = cas(s, key);
    if (was == kEmptyKey || was == key) return s;
  }
  return kNone;
}
template <class Keys>
MNAV_HD uint32_t sep_find(const Keys* keys, uint32_t mask, uint64_t key)
{
  uint32_t s = sep_hash(key, mask);
  for (uint32_t probes = 0; probes <= mask; ++probes, s = (s + 1) & mask) {
    const uint64_t k = (uint64_t)keys[s];
    if (k == key) return s;
    if (k == kEmptyKey) return kNone;
  }
  return kNone;
}

// the rule: departure, presence, distance, a partner, the end of a check.  tick: a call tick, from 1
MNAV_HD bool frol_waits(uint32_t tick, uint32_t start_tick) { return tick <= start_tick; }
MNAV_HD bool sep_present(int32_t status, bool waiting, uint32_t flags, W3 p)
{
  if (!(sep_finite(p.x) && sep_finite(p.y) && sep_finite(p.z))) return false;
  if (status == mnav_rol::kRunning) return !waiting || (flags & kWaitingPresent) != 0;
  if (status == mnav_rol::kReached) return (flags & kReachedPresent) != 0;
  return true;                                                        // OUT_OF_MAP, NO_FIELD: a stranded robot is an obstacle
}
MNAV_HD float sep_d2(W3 a, W3 b)
{
  const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float xy = xx + yy;
  return xy + zz;
}
MNAV_HD Row sep_row_start()
{
  Row R;
  R.near_checks = 0; R.max_partners = 0; R.first_near_tick = kNone; R.first_near_robot = kNone; R.min_sep2 = INFINITY; R.min_sep_tick = kNone; R.min_sep_robot = kNone;
  return R;
}
MNAV_HD Best sep_best_start() { Best b; b.partners = 0; b.d2 = INFINITY; b.id = kNone; return b; }
MNAV_HD void sep_meet(Best& b, float d2, uint32_t j)
{
  b.partners += 1;
  if (d2 < b.d2 || (d2 == b.d2 && j < b.id)) { b.d2 = d2; b.id = j; }
}
MNAV_HD void sep_close(Row& R, const Best& b, uint32_t tick)
{
  if (!b.partners) return;
  R.near_checks += 1;
  if (b.partners > R.max_partners) R.max_partners = b.partners;
  if (R.first_near_tick == kNone) { R.first_near_tick = tick; R.first_near_robot = b.id; }
  if (b.d2 < R.min_sep2) { R.min_sep2 = b.d2; R.min_sep_tick = tick; R.min_sep_robot = b.id; }
}

// The one walk over the cells of the range of a robot at p: cell(slot) for every cell of it that exists.
template <class Keys, class Cell>
MNAV_HD void sep_cells(const Grid& G, const Keys* keys, uint32_t mask, W3 p, Cell cell)
{
  const Range R = sep_range(G, p);
  for (int cx = R.lo[0]; cx <= R.hi[0]; ++cx)
    for (int cy = R.lo[1]; cy <= R.hi[1]; ++cy)
      for (int cz = R.lo[2]; cz <= R.hi[2]; ++cz) {
        const uint32_t s = sep_find(keys, mask, sep_key(cx, cy, cz));
        if (s != kNone) cell(s);
      }
}
// the populations of those cells: the distance tests sep_near performs for the robot (its own record among them)
template <class Keys>
MNAV_HD uint64_t sep_tests(const Grid& G, const Keys* keys, uint32_t mask, const uint32_t* cnt, W3 p)
{
  uint64_t tests = 0;
  sep_cells(G, keys, mask, p, [&](uint32_t s) { tests += cnt[s]; });
  return tests;
}
// Every record of those cells but robot i's own whose d2 <= r2 goes to near(j, d2, pj).  rec: 4 floats per record, (x, y, z,
// the id's bits), sorted by slot; cnt / start: per slot.
template <class Keys, class Near>
MNAV_HD void sep_near(const Grid& G, const Keys* keys, uint32_t mask, const uint32_t* cnt, const uint32_t* start, const float* rec, uint32_t i, W3 p, Near near)
{
  sep_cells(G, keys, mask, p, [&](uint32_t s) {
    const uint32_t c = cnt[s];
    const float* q = rec + 4 * (size_t)start[s];
    for (uint32_t k = 0; k < c; ++k, q += 4) {
      const uint32_t j = sep_bits(q[3]);
      if (j == i) continue;
      const W3 pj = mnav::w3(q[0], q[1], q[2]);
      const float d2 = sep_d2(p, pj);
      if (d2 <= G.r2) near(j, d2, pj);
    }
  });
}

// the per-robot outputs as arrays (device or host)
struct Rows {
  uint32_t* near_checks; uint32_t* max_partners; uint32_t* first_near_tick; uint32_t* first_near_robot; float* min_sep2; uint32_t* min_sep_tick; uint32_t* min_sep_robot;
};
MNAV_HD Row sep_row_load(const Rows& A, uint32_t i)
{
  Row R;
  R.near_checks = A.near_checks[i]; R.max_partners = A.max_partners[i]; R.first_near_tick = A.first_near_tick[i]; R.first_near_robot = A.first_near_robot[i];
  R.min_sep2 = A.min_sep2[i]; R.min_sep_tick = A.min_sep_tick[i]; R.min_sep_robot = A.min_sep_robot[i];
  return R;
}
MNAV_HD void sep_row_store(const Rows& A, uint32_t i, const Row& R)
{
  A.near_checks[i] = R.near_checks; A.max_partners[i] = R.max_partners; A.first_near_tick[i] = R.first_near_tick; A.first_near_robot[i] = R.first_near_robot;
  A.min_sep2[i] = R.min_sep2; A.min_sep_tick[i] = R.min_sep_tick; A.min_sep_robot[i] = R.min_sep_robot;
}

// the table for n robots: the smallest power of two >= max(2 n, 64)
inline uint32_t sep_table_size(uint32_t n)
{
  uint64_t m = 64;
  while (m < 2 * (uint64_t)n) m <<= 1;
  return (uint32_t)m;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The host mirrors of a check, serially, over the same pieces.  HostGrid: what the device passes up to k_sep_fill leave of
// call tick `tick` (from 1), positions and statuses as they stand after it.  table_size: a power of two > n.
struct HostGrid {
  uint32_t mask; uint64_t tests = 0, max_cell = 0;
  std::vector<uint64_t> keys; std::vector<uint32_t> cnt, start, slot_of, rank; std::vector<float> rec;
  HostGrid(uint32_t n, const float* pos, const int32_t* status, const uint32_t* start_tick, uint32_t tick, uint32_t flags, const Grid& G, uint32_t table_size)
      : mask(table_size - 1), keys(table_size, kEmptyKey), cnt(table_size, 0u), start(table_size), slot_of(n, kNone), rank(n), rec(4 * (size_t)n)
  {
    for (uint32_t i = 0; i < n; ++i) {
      const W3 p = mnav::w3_load(pos + 3 * (size_t)i);
      if (!sep_present(status[i], start_tick && frol_waits(tick, start_tick[i]), flags, p)) continue;
      const uint32_t s = sep_insert(mask, sep_key_of(G, p), [&](uint32_t at, uint64_t key) { const uint64_t was = keys[at]; if (was == kEmptyKey) keys[at] = key; return was; });
      slot_of[i] = s; rank[i] = cnt[s]++;
    }
    uint32_t sum = 0;
    for (uint32_t s = 0; s < table_size; ++s) { start[s] = sum; sum += cnt[s]; }
    for (uint32_t i = 0; i < n; ++i) {
      if (slot_of[i] == kNone) continue;
      const W3 p = mnav::w3_load(pos + 3 * (size_t)i);
      float* q = rec.data() + 4 * (size_t)(start[slot_of[i]] + rank[i]);
      q[0] = p.x; q[1] = p.y; q[2] = p.z; q[3] = sep_float(i);
      if (cnt[slot_of[i]] > max_cell) max_cell = cnt[slot_of[i]];
      tests += sep_tests(G, keys.data(), mask, cnt.data(), p);        // (keys and counts are final: only the records are being placed)
    }
  }
};
// One check: the check's row chk (kCheckWords), the guard, and for every present robot robot(grid, i, b) -- which meets the
// robot's partners into b -- and b into the robot's Row.  Returns false when the guard skipped the pair pass: no robot ran.
template <class Robot>
inline bool sep_check_host_each(uint32_t n, const float* pos, const int32_t* status, const uint32_t* start_tick, uint32_t tick, uint32_t flags, const Grid& G,
                                uint32_t table_size, uint64_t max_tests, const Rows& rows, uint64_t* chk, Robot robot)
{
  const HostGrid H(n, pos, status, start_tick, tick, flags, G, table_size);
  chk[kChkTests] = H.tests; chk[kChkMaxCell] = H.max_cell; chk[kChkOrdered] = 0; chk[kChkSkipped] = H.tests > max_tests;
  if (chk[kChkSkipped]) return false;
  for (uint32_t i = 0; i < n; ++i) {
    if (H.slot_of[i] == kNone) continue;
    Best b = sep_best_start();
    robot(H, i, b);
    Row R = sep_row_load(rows, i);
    sep_close(R, b, tick);
    sep_row_store(rows, i, R);
    chk[kChkOrdered] += b.partners;
  }
  return true;
}
// the mirror of k_sep_clear .. k_sep_pair
inline bool sep_check_host(uint32_t n, const float* pos, const int32_t* status, const uint32_t* start_tick, uint32_t tick, uint32_t flags, const Grid& G,
                           uint32_t table_size, uint64_t max_tests, const Rows& rows, uint64_t* chk)
{
  return sep_check_host_each(n, pos, status, start_tick, tick, flags, G, table_size, max_tests, rows, chk, [&](const HostGrid& H, uint32_t i, Best& b) {
    sep_near(G, H.keys.data(), H.mask, H.cnt.data(), H.start.data(), H.rec.data(), i, mnav::w3_load(pos + 3 * (size_t)i), [&](uint32_t j, float d2, W3) { sep_meet(b, d2, j); });
  });
}
#endif

// What a call tells of its checks afterwards (mnav_fleet_rollout_stats); `= {}` is the reset, the values of a call without
// a check.
struct SepStats {
  uint32_t checks_run = 0, checks_skipped = 0, first_skipped_tick = kNone, robots_near = 0, max_pairs_tick = kNone, min_pair[2] = { kNone, kNone }, max_cell = 0;
  uint64_t near_pairs = 0, max_pairs = 0, tests = 0; float min_sep2 = INFINITY;
  float ms_separation = 0.f;
};

// The check rows of the `checks` checks a call of n robots ran (check c after call tick (c + 1) * check_stride) and three of
// the rows' columns, folded into a reset S, on the host (plain C++, as rol_fold_counters).  A skipped check counts, with the first one's tick, and its largest cell counts;
// its tests and pairs do not.  The first check with the most pairs gives max_pairs_tick, the smallest index min_pair.
inline void sep_fold(const uint64_t* chk, uint32_t checks, uint32_t check_stride, uint32_t n, const uint32_t* near_checks, const float* min_sep2,
                     const uint32_t* min_sep_robot, SepStats& S)
{
  for (uint32_t c = 0; c < checks; ++c) {
    const uint64_t* row = chk + (size_t)kCheckWords * c;
    const uint32_t tick = (c + 1) * check_stride;
    if (row[kChkMaxCell] > S.max_cell) S.max_cell = (uint32_t)row[kChkMaxCell];
    if (row[kChkSkipped]) { if (!S.checks_skipped++) S.first_skipped_tick = tick; continue; }
    S.checks_run += 1; S.tests += row[kChkTests];
    const uint64_t pairs = row[kChkOrdered] / 2;                      // every near pair was met from both sides
    S.near_pairs += pairs;
    if (S.max_pairs_tick == kNone || pairs > S.max_pairs) { S.max_pairs = pairs; S.max_pairs_tick = tick; }
  }
  for (uint32_t i = 0; i < n; ++i) {
    if (near_checks[i]) S.robots_near += 1;
    if (min_sep2[i] < S.min_sep2) { S.min_sep2 = min_sep2[i]; S.min_pair[0] = i; S.min_pair[1] = min_sep_robot[i]; }   // the smallest i: its partner is larger
  }
}

#if defined(__HIPCC__)

constexpr int kSepBlock = 256;     // lanes per workgroup of every pass of a check
constexpr int kSepPer = 8;         // slots per lane of the scan: tiles of kSepBlock * kSepPer slots
constexpr uint32_t kSepTile = kSepBlock * kSepPer;

// The rollout's tick with a departure: robot i has no tick before device tick start_tick[i] (never null: a call without
// start ticks runs k_rollout_*).
struct FleetTick : mnav_rol::Tick {
  const uint32_t* start_tick; uint32_t tick;

  __device__ __forceinline__ FleetTick(const mnav_rol::Batch& B, const mnav_rol::Params& P_, uint32_t tick_, uint32_t trace_row_, const uint32_t* start_tick_)
      : mnav_rol::Tick(B, P_, tick_, trace_row_), start_tick(start_tick_), tick(tick_) {}
  __device__ __forceinline__ bool first(uint32_t ic, uint32_t& f, W3& p) const
  {
    const bool running = mnav_rol::Tick::first(ic, f, p);
    return running && !frol_waits(tick + 1, start_tick[ic]);
  }
};

__global__ __launch_bounds__(mnav_fol::kStayBlock) void k_fleet_rollout_stay(mnav_rol::Batch B, mnav::WalkMesh M, mnav_fol::Config C, mnav_rol::Params P, uint32_t tick,
                                                                              uint32_t trace_row, const uint32_t* start_tick)
{
  mnav_fol::fol_pass_stay(FleetTick(B, P, tick, trace_row, start_tick), M, C);
}

__global__ __launch_bounds__(64) void k_fleet_rollout_search(mnav_rol::Batch B, mnav::WalkMesh M, mnav_fol::Config C, mnav_rol::Params P, uint32_t tick,
                                                             uint32_t trace_row, const uint32_t* start_tick)
{
  __shared__ uint32_t list[mnav::kWalkScratchWords];
  mnav_fol::fol_pass_search(FleetTick(B, P, tick, trace_row, start_tick), M, C, list);
}

__global__ __launch_bounds__(mnav_loc::kLocBlock) void k_fleet_rollout_global(mnav_rol::Batch B, mnav::WalkMesh M, mnav_fol::Config C, mnav_rol::Params P,
                                                                              mnav_loc::Index I, uint32_t tick, uint32_t trace_row, const uint32_t* start_tick)
{
  __shared__ uint32_t s_node[mnav_loc::kStack * mnav_loc::kLocBlock];
  __shared__ float s_bound[mnav_loc::kStack * mnav_loc::kLocBlock];
  const FleetTick T(B, P, tick, trace_row, start_tick);
  mnav_fol::fol_pass_global(T, M, C, I, T.cnt[1] < T.n ? T.cnt[1] : T.n, s_node, s_bound);
}

// what the passes of a check see
struct Sep {
  uint32_t n, flags, mask, tiles; Grid G; unsigned long long max_tests;
  const float* pos; const int32_t* status; const uint32_t* start_tick;           // start_tick: may be null
  unsigned long long* keys; uint32_t* cnt; uint32_t* start; uint32_t* tile;       // the table (mask + 1 slots), the tile sums / offsets
  uint32_t* slot_of; uint32_t* rank; float* rec;                                 // per robot; rec: 4 floats per present robot, sorted by slot
  unsigned long long* chk;                                                       // the call's check rows (kCheckWords each)
  Rows rows;
};

__device__ __forceinline__ unsigned long long sep_wave_sum(unsigned long long v)
{
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}
__device__ __forceinline__ uint32_t sep_wave_max(uint32_t v)
{
  for (int off = 32; off > 0; off >>= 1) { const uint32_t u = (uint32_t)__shfl_xor((int)v, off); v = u > v ? u : v; }
  return v;
}
// exclusive scan of one value per lane over the workgroup; *total: its sum
__device__ __forceinline__ uint32_t sep_block_scan(uint32_t v, uint32_t* lds, uint32_t* total)
{
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint32_t s = v;
  for (int off = 1; off < 64; off <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)s, off); if (lane >= (uint32_t)off) s += u; }
  if (lane == 63) lds[w] = s;
  __syncthreads();
  uint32_t base = 0, all = 0;
  for (uint32_t k = 0; k < kSepBlock / 64; ++k) { if (k < w) base += lds[k]; all += lds[k]; }
  __syncthreads();
  *total = all;
  return base + s - v;
}

__global__ __launch_bounds__(kSepBlock) void k_sep_clear(Sep S)
{
  for (size_t s = (size_t)blockIdx.x * kSepBlock + threadIdx.x; s <= S.mask; s += (size_t)gridDim.x * kSepBlock) { S.keys[s] = kEmptyKey; S.cnt[s] = 0; }
}

__global__ __launch_bounds__(kSepBlock) void k_sep_insert(Sep S, uint32_t tick)
{
  const uint32_t i = blockIdx.x * kSepBlock + threadIdx.x;
  if (i >= S.n) return;
  const W3 p = mnav::w3_load(S.pos + 3 * (size_t)i);
  uint32_t slot = kNone;
  if (sep_present(S.status[i], S.start_tick && frol_waits(tick, S.start_tick[i]), S.flags, p)) {
    unsigned long long* keys = S.keys;
    slot = sep_insert(S.mask, sep_key_of(S.G, p), [keys](uint32_t at, uint64_t key) { return (uint64_t)atomicCAS(&keys[at], (unsigned long long)kEmptyKey, (unsigned long long)key); });
    if (slot != kNone) S.rank[i] = atomicAdd(&S.cnt[slot], 1u);       // (the table holds more slots than robots: a slot is always found)
  }
  S.slot_of[i] = slot;
}

// the scan of the counts: tile sums, their exclusive scan by one workgroup, every tile over its own counts
__global__ __launch_bounds__(kSepBlock) void k_sep_sums(Sep S)
{
  __shared__ uint32_t lds[kSepBlock / 64];
  const size_t s0 = ((size_t)blockIdx.x * kSepBlock + threadIdx.x) * kSepPer;
  uint32_t c = 0;
  for (int k = 0; k < kSepPer; ++k) if (s0 + k <= S.mask) c += S.cnt[s0 + k];
  uint32_t total;
  (void)sep_block_scan(c, lds, &total);
  if (threadIdx.x == 0) S.tile[blockIdx.x] = total;
}
__global__ __launch_bounds__(kSepBlock) void k_sep_top(Sep S)
{
  __shared__ uint32_t lds[kSepBlock / 64];
  uint32_t carry = 0;
  for (uint32_t b0 = 0; b0 < S.tiles; b0 += kSepBlock) {
    const uint32_t b = b0 + threadIdx.x, v = b < S.tiles ? S.tile[b] : 0u;
    uint32_t total;
    const uint32_t ex = sep_block_scan(v, lds, &total);
    if (b < S.tiles) S.tile[b] = carry + ex;
    carry += total;
  }
}
__global__ __launch_bounds__(kSepBlock) void k_sep_starts(Sep S)
{
  __shared__ uint32_t lds[kSepBlock / 64];
  const size_t s0 = ((size_t)blockIdx.x * kSepBlock + threadIdx.x) * kSepPer;
  uint32_t c[kSepPer], sum = 0;
  for (int k = 0; k < kSepPer; ++k) { c[k] = s0 + k <= S.mask ? S.cnt[s0 + k] : 0u; sum += c[k]; }
  uint32_t total;
  uint32_t at = S.tile[blockIdx.x] + sep_block_scan(sum, lds, &total);
  for (int k = 0; k < kSepPer; ++k) if (s0 + k <= S.mask) { S.start[s0 + k] = at; at += c[k]; }
}

__global__ __launch_bounds__(kSepBlock) void k_sep_fill(Sep S, uint32_t check)
{
  const uint32_t i = blockIdx.x * kSepBlock + threadIdx.x;
  unsigned long long tests = 0;
  uint32_t cell = 0;
  if (i < S.n) {
    const uint32_t slot = S.slot_of[i];
    if (slot != kNone) {
      const W3 p = mnav::w3_load(S.pos + 3 * (size_t)i);
      float* q = S.rec + 4 * (size_t)(S.start[slot] + S.rank[i]);     // start + rank < the present robots <= n
      q[0] = p.x; q[1] = p.y; q[2] = p.z; q[3] = sep_float(i);
      cell = S.cnt[slot];
      tests = sep_tests(S.G, S.keys, S.mask, S.cnt, p);
    }
  }
  tests = sep_wave_sum(tests);
  cell = sep_wave_max(cell);
  if ((threadIdx.x & 63u) == 0) {
    unsigned long long* row = S.chk + (size_t)kCheckWords * check;
    if (tests) atomicAdd(&row[kChkTests], tests);
    if (cell) atomicMax(&row[kChkMaxCell], (unsigned long long)cell);
  }
}

__global__ __launch_bounds__(kSepBlock) void k_sep_pair(Sep S, uint32_t check, uint32_t tick)
{
  unsigned long long* row = S.chk + (size_t)kCheckWords * check;
  if (row[kChkTests] > S.max_tests) {                                 // (final: k_sep_fill has ended; uniform over the grid)
    if (blockIdx.x == 0 && threadIdx.x == 0) row[kChkSkipped] = 1;
    return;
  }
  const uint32_t i = blockIdx.x * kSepBlock + threadIdx.x;
  unsigned long long partners = 0;
  if (i < S.n && S.slot_of[i] != kNone) {
    Best b = sep_best_start();
    sep_near(S.G, S.keys, S.mask, S.cnt, S.start, S.rec, i, mnav::w3_load(S.pos + 3 * (size_t)i), [&](uint32_t j, float d2, W3) { sep_meet(b, d2, j); });
    if (b.partners) {
      Row R = sep_row_load(S.rows, i);
      sep_close(R, b, tick);
      sep_row_store(S.rows, i, R);
    }
    partners = b.partners;
  }
  partners = sep_wave_sum(partners);
  if ((threadIdx.x & 63u) == 0 && partners) atomicAdd(&row[kChkOrdered], partners);
}

// what a fleet rollout adds on the device to mnav_rol::Dev (grown on demand, kept between calls): the start ticks, the
// check's table, records, separation rows and check rows, and the event pairs that time the checks of a block
struct State {
  mnav::DevBuf<uint32_t> start_tick, cell_cnt, cell_start, tile, slot_of, rank, near_checks, max_partners, first_near_tick, first_near_robot, min_sep_tick, min_sep_robot;
  mnav::DevBuf<float> rec, min_sep2; mnav::DevBuf<unsigned long long> keys, chk;
  size_t cap = 0, sep_cap = 0, table_cap = 0, chk_cap = 0;
  mnav::Event ev[2 * mnav_rol::kBlockTicks]; bool have_ev = false;
};

#endif  // __HIPCC__

}  // namespace mnav_frol
