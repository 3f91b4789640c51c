// mnav_schedule.h -- fleet schedule (mnav_fleet_schedule, mnav_schedule_stats): a departure delay per robot, in whole
// windows, such that no (vertex, window) cell holds more than `capacity`.  The cells are the timed
// cells of mnav_timed.h -- V x B uint32 cells and holders, T -- and the robots, the contributor rule and the float32 window
// arithmetic (timed_time, timed_slot) are the timed call's.
// A contributor i tries delay d with depart_d = depart_i + (float) d * (float) tau (one multiply, then one add, no
// contraction: d = 0 gives depart_i bit for bit).  Its len + 1 visits then fall at t = timed_time(P, dist[u], depart_d,
// pace_i) into timed_slot(t, tau, B).  Candidate d FITS iff every visit lies inside the horizon and every CONSTRAINED visit
// has cell[u][k] + w_i <= capacity; every visit is constrained but, under MNAV_SCHEDULE_SEED_FREE, the last one (on the
// seed).  The float operations are monotone in d: once a candidate has a visit beyond the horizon every larger one has too.
// Rounds r = 1, 2, ... on the committed cells and a current delay `cur` per robot (0 at the start):
//   probe   every OPEN robot takes the smallest d in [cur, max_delay] that fits the cells as they stand at the start of
//           the round and sets cur = d; none fits: NO_SLOT, for good (cells only grow)
//   claim   every robot that found a d adds w_i to tent[u][k] of each constrained visit and lowers the tentative holder
//           of the cell to (key_i, i), ordered lexicographically
//   decide  a robot WINS iff for every constrained visit cell + tent <= capacity or the tentative holder is the robot
//   commit  every winner is COMMITTED with delay d in round r: ALL its visits (the seed's too) add w_i to the cell and
//           lower the holder to key_i, T grows by w_i; losers stay OPEN and probe again from cur
// until nobody is OPEN or r == max_rounds.  The tentative arrays are clean at the start of every round.  Integer sums and
// minima do not depend on their order: outputs and cells are the same bits on every schedule of the atomics, with any
// chunking of the rounds and either way of cleaning the tentative arrays.
// NOT claimed: the result is not the sequential "robots in key order" greedy schedule -- the rule above is its own
// definition; and scheduling two halves of a fleet in two accumulating calls is not the same as one call over the whole
// fleet (the first half never sees the second), unlike counting.
// schedule_depart, schedule_full, schedule_ticket, schedule_refusal and -- over fleet_classify -- schedule_host are the
// device's own source and the host mirror's (tests/test_fleet_schedule_model.py).
//
// Device shape: classification and hop counts are k_fleet_cut / k_fleet_len of mnav_fleet.h, unchanged.  The OPEN robots
// of a round are a dense list (two lists, swapped every round; the losers of the commit pass append themselves to the
// next one, in any order: no result depends on it).  k_schedule_probe: one wave per OPEN robot, lane g = candidate cur + g;
// per hop pred[u] and dist[u] are wave-uniform loads through GPtr, each lane computes its own window and reads
// cell[u * B + k_g] -- neighbouring candidates land in neighbouring or equal windows, one contiguous run of the vertex's
// row; lanes beyond max_delay are masked, a ballot of the lanes that still fit ends the walk when it is empty, the lowest
// fitting lane is the answer, and a wave whose 64 candidates are exhausted inside the horizon walks again for the next 64.
// k_schedule_claim / _decide / _commit: one lane per OPEN robot walks its len + 1 visits as k_timed_add does; claim and commit
// use no-return atomicAdd / atomicMin (64-bit on key << 32 | index for the tentative holder); the commit pass also cleans
// the claimants' tentative words (plain stores of the clean value) unless the host fills the arrays between the rounds.
// k_schedule_next: one lane folds the round's counters into the control record; every kernel of a round reads the record's
// (round, open) -- which only k_schedule_next writes -- and returns at once when open == 0 or the round limit is reached,
// so the host enqueues rounds in chunks without looking.  No kernel waits for another workgroup; every walk is bounded by
// the len the classification counted.
#pragma once
#include <cmath>
#include <cstdint>

#include "mnav_timed.h"

namespace mnav_schedule {

using mnav_fleet::Field;
using mnav_fleet::Robot;
using mnav_timed::timed_slot;
using mnav_timed::timed_time;
using mnav_traffic::traffic_contributes;

constexpr int kScheduleBlock = 256;                       // lanes per block: 256 robots, or 4 robots in the probe
constexpr uint32_t kChunkRounds = 8u;                     // default of the option schedule_chunk_rounds
constexpr uint32_t kSeedFree = 1u;                        // MNAV_SCHEDULE_SEED_FREE
constexpr uint32_t kBytesPerCell = 20u;                   // cell, holder, tentative count (4 each), tentative holder (8)
enum { kStNone = 0, kStCommitted = 1, kStNoSlot = 2, kStOpen = 3 };
constexpr unsigned long long kNoTicket = ~0ull;           // the clean tentative holder

// the departure of candidate d: one multiply, then one add
MNAV_HD float schedule_depart(float depart, uint32_t d, float tau)
{
  const float wait = (float)d * tau;
  return depart + wait;
}
// does a cell that holds `have` refuse w more under `capacity`?  (w <= capacity: no wrap)
MNAV_HD bool schedule_full(uint32_t have, uint32_t w, uint32_t capacity) { return have > capacity - w; }
// the order of the tentative holders: by key, then by robot index
MNAV_HD unsigned long long schedule_ticket(uint32_t key, uint32_t i) { return ((unsigned long long)key << 32) | i; }

// what the schedule refuses on top of timed_refusal (null: nothing)
inline const char* schedule_refusal(uint32_t B, uint32_t capacity, uint32_t max_delay, uint32_t flags)
{
  if (capacity < 1u) return "capacity must be at least 1";
  if (max_delay >= B) return "max_delay must be below windows";
  if (flags & ~kSeedFree) return "unknown flag bit";
  return nullptr;
}

// the counters of one call (host copy of the device's control record)
struct Counts {
  uint32_t round, open, committed, no_slot, contributing, delayed, max_delay_used;
  uint32_t pend_won, pend_no_slot, pend_next, pad;                   // of the round in flight: folded by k_schedule_next
  unsigned long long claims, visits, weight;
};

#if !defined(__HIP_DEVICE_COMPILE__)
// mnav_fleet_schedule on host arrays: `fields` with host pointers and their cuts set; cell / holder (V x B words), *T, peak /
// window (V words) the context's state, whose configuration is (state_B, state_tau) when it has one.  Returns -1 with
// nothing touched on a refusal.  Per robot (any may be null): code, potential, status, delay, depart_out, round; counts: the
// call's counters; words: mnav_timed's kWords of the cells afterwards; per_round: (claimed, won) of the first per_round_cap
// rounds.
inline int schedule_host(uint32_t n, uint32_t V, const Field* fields, const uint32_t* slot, const uint32_t* vtx, const uint32_t* weights, const float* depart,
                         const float* pace, const uint32_t* key, uint32_t B, double tau, uint32_t capacity, uint32_t max_delay, uint32_t max_rounds,
                         uint32_t flags, int accumulate, uint32_t state_B, float state_tau, uint32_t* cell, uint32_t* holder, unsigned long long* T,
                         uint32_t* peak, uint32_t* window, uint32_t* code, float* potential, uint32_t* status, uint32_t* delay, float* depart_out,
                         uint32_t* round, Counts* counts, unsigned long long* words, uint32_t* per_round, uint32_t per_round_cap)
{
  if (mnav_timed::timed_refusal(n, weights, depart, pace, B, tau, accumulate, *T, state_B, state_tau)) return -1;
  if (schedule_refusal(B, capacity, max_delay, flags)) return -1;
  const float tf = (float)tau;
  const size_t cells = (size_t)V * B;
  if (!accumulate) { for (size_t c = 0; c < cells; ++c) { cell[c] = 0u; holder[c] = mnav::kNone; } *T = 0ull; }
  struct Seen { uint32_t len, w, key, cur, st, rnd; float P, dep, pc; bool win; };
  Seen* R = new Seen[n ? n : 1];
  uint32_t* tent = new uint32_t[cells ? cells : 1];
  unsigned long long* thold = new unsigned long long[cells ? cells : 1];
  for (size_t c = 0; c < cells; ++c) { tent[c] = 0u; thold[c] = kNoTicket; }
  Counts K = {};
  for (uint32_t i = 0; i < n; ++i) {
    const Field& Fd = fields[slot[i]];
    Robot C = mnav_fleet::fleet_classify(Fd, V, vtx[i]);
    if (C.unreached) {                                                // rule 5 under a finite cut: did the wave run out?
      bool open = false;
      for (uint32_t u = 0; u < V && !open; ++u) open = mnav_fleet::fleet_open_value(Fd.dist[u], Fd.cut);
      if (!open) C.code = mnav_fleet::kNoPath;
    }
    if (code) code[i] = C.code;
    if (potential) potential[i] = C.potential;
    Seen& S = R[i];
    S.len = C.len; S.P = C.potential; S.w = weights ? weights[i] : 1u; S.key = key ? key[i] : i; S.dep = depart ? depart[i] : 0.f; S.pc = pace ? pace[i] : 1.f;
    S.cur = 0u; S.rnd = mnav::kNone; S.win = false;
    S.st = traffic_contributes(C.code, C.potential) && S.w ? kStOpen : kStNone;
    K.contributing += S.st == kStOpen;
  }
  K.open = K.contributing;
  // visit q of robot i at delay d: false beyond the horizon
  auto visit = [&](uint32_t i, uint32_t d, uint32_t u, size_t* c) {
    uint32_t k;
    if (!timed_slot(timed_time(R[i].P, fields[slot[i]].dist[u], schedule_depart(R[i].dep, d, tf), R[i].pc), tf, B, &k)) return false;
    *c = (size_t)u * B + k;
    return true;
  };
  while (K.open && (!max_rounds || K.round < max_rounds)) {
    uint32_t claimed = 0u, won = 0u;
    for (uint32_t i = 0; i < n; ++i) {                                  // probe
      Seen& S = R[i];
      if (S.st != kStOpen) continue;
      bool found = false;
      for (uint32_t d = S.cur; d <= max_delay && S.w <= capacity && !found; ++d) {
        bool fits = true, beyond = false;
        uint32_t u = vtx[i];
        for (uint32_t q = 0; q <= S.len && fits; ++q) {
          size_t c;
          if (!visit(i, d, u, &c)) { fits = false; beyond = true; }
          else if (!((flags & kSeedFree) && q == S.len) && schedule_full(cell[c], S.w, capacity)) fits = false;
          u = fields[slot[i]].pred[u];
        }
        if (fits) { S.cur = d; found = true; }
        else if (beyond) break;                                       // every larger delay is beyond the horizon too
      }
      if (!found) { S.st = kStNoSlot; ++K.no_slot; --K.open; }
    }
    for (uint32_t i = 0; i < n; ++i) {                                  // claim
      const Seen& S = R[i];
      if (S.st != kStOpen) continue;
      ++claimed;
      uint32_t u = vtx[i];
      for (uint32_t q = 0; q <= S.len; ++q) {
        size_t c = 0;
        visit(i, S.cur, u, &c);
        if (!((flags & kSeedFree) && q == S.len)) {
          tent[c] += S.w;
          const unsigned long long tk = schedule_ticket(S.key, i);
          if (tk < thold[c]) thold[c] = tk;
        }
        u = fields[slot[i]].pred[u];
      }
    }
    for (uint32_t i = 0; i < n; ++i) {                                  // decide
      Seen& S = R[i];
      if (S.st != kStOpen) continue;
      S.win = true;
      uint32_t u = vtx[i];
      for (uint32_t q = 0; q <= S.len; ++q) {
        size_t c = 0;
        visit(i, S.cur, u, &c);
        if (!((flags & kSeedFree) && q == S.len) && (unsigned long long)cell[c] + tent[c] > capacity && thold[c] != schedule_ticket(S.key, i)) S.win = false;
        u = fields[slot[i]].pred[u];
      }
    }
    for (uint32_t i = 0; i < n; ++i) {                                  // commit, and the claimants clean their tentative words
      Seen& S = R[i];
      if (S.st != kStOpen) continue;
      uint32_t u = vtx[i];
      for (uint32_t q = 0; q <= S.len; ++q) {
        size_t c = 0;
        visit(i, S.cur, u, &c);
        if (S.win) { cell[c] += S.w; if (S.key < holder[c]) holder[c] = S.key; }
        tent[c] = 0u; thold[c] = kNoTicket;
        u = fields[slot[i]].pred[u];
      }
      if (!S.win) continue;
      S.st = kStCommitted; S.rnd = K.round + 1u;
      ++won; ++K.committed; --K.open; K.visits += (unsigned long long)S.len + 1ull; K.weight += S.w;
      K.delayed += S.cur > 0u; if (S.cur > K.max_delay_used) K.max_delay_used = S.cur;
    }
    if (per_round && K.round < per_round_cap) { per_round[2 * (size_t)K.round] = claimed; per_round[2 * (size_t)K.round + 1] = won; }
    K.claims += claimed;
    ++K.round;
  }
  *T += K.weight;
  unsigned long long s[mnav_timed::kWords] = {};
  s[mnav_timed::kContributing] = K.committed; s[mnav_timed::kAdds] = K.visits; s[mnav_timed::kWeight] = K.weight;
  mnav_timed::timed_peak_host(V, B, cell, capacity, peak, window, s);
  for (uint32_t i = 0; i < n; ++i) {
    const bool done = R[i].st == kStCommitted;
    if (status) status[i] = R[i].st;
    if (delay) delay[i] = done ? R[i].cur : mnav::kNone;
    if (depart_out) depart_out[i] = done ? schedule_depart(R[i].dep, R[i].cur, tf) : mnav::inf_f();
    if (round) round[i] = R[i].rnd;
  }
  delete[] R; delete[] tent; delete[] thold;
  if (counts) *counts = K;
  if (words) for (int k = 0; k < mnav_timed::kWords; ++k) words[k] = s[k];
  return 0;
}
#endif

#if defined(__HIPCC__)

// one call as its kernels see it
struct Job {
  uint32_t n, V, B; float tau; uint32_t capacity, max_delay, limit, flags, undo;   // limit: rounds; undo: the commit pass cleans the tentative words
  const uint32_t* slot; const uint32_t* vtx; const Field* fields;
  const uint32_t* code; const uint32_t* len; const float* potential;   // of k_fleet_len (a later k_fleet_resolve moves no MNAV_SUCCESS)
  const uint32_t* weight; const float* depart; const float* pace; const uint32_t* key;   // null: 1, 0, 1, the robot's index
  uint32_t* cell; uint32_t* holder; uint32_t* tent; unsigned long long* thold;
  Counts* ctl; uint32_t* list;                                         // 2 x n: the OPEN robots of even and of odd rounds
  uint32_t* st; uint32_t* cur; uint32_t* win;                          // per robot
  uint32_t* delay_out; uint32_t* round_out; float* depart_out;         // per robot: MNAV_NONE / MNAV_NONE / +inf unless committed
};

// is there a round to run?  (round and open are written by k_schedule_next alone: every lane of a round's kernels agrees)
__device__ __forceinline__ bool schedule_active(const Job& J, uint32_t* open, uint32_t* round)
{
  const mnav::GPtr<const Counts> K(J.ctl);
  *open = K->open; *round = K->round;
  return *open != 0u && *round < J.limit;
}

// robot i (< n) as a walk sees it
struct Lane { uint32_t u, len, w, key; float P, depart, pace; mnav::GPtr<const float> dist; mnav::GPtr<const uint32_t> pred; };
__device__ __forceinline__ Lane schedule_lane(const Job& J, uint32_t i)
{
  const uint32_t s = J.slot[i], v = J.vtx[i], last = J.V - 1u;
  Lane L;
  L.P = J.potential[i]; L.len = J.len[i];
  L.w = J.weight ? J.weight[i] : 1u;                                  // (wave-uniform branches)
  L.depart = J.depart ? J.depart[i] : 0.f;
  L.pace = J.pace ? J.pace[i] : 1.f;
  L.key = J.key ? J.key[i] : i;
  L.dist = J.fields[s].dist; L.pred = J.fields[s].pred;
  L.u = v < last ? v : last;                                          // a contributor stands on a vertex (rule 1)
  return L;
}

// statuses, delays and outputs of all n robots; the contributors form the first list
__global__ __launch_bounds__(kScheduleBlock) void k_schedule_init(Job J)
{
  const uint32_t i = blockIdx.x * kScheduleBlock + threadIdx.x, lane = threadIdx.x & 63u;
  const uint32_t j = i < J.n ? i : J.n - 1u;                          // clamped (n >= 1): the loads are unconditional
  const uint32_t w = J.weight ? J.weight[j] : 1u;
  const bool on = i < J.n && w != 0u && traffic_contributes(J.code[j], J.potential[j]);
  if (i < J.n) {
    J.st[i] = on ? (uint32_t)kStOpen : (uint32_t)kStNone; J.cur[i] = 0u; J.win[i] = 0u;
    J.delay_out[i] = mnav::kNone; J.round_out[i] = mnav::kNone; J.depart_out[i] = mnav::inf_f();
  }
  const unsigned long long m = __ballot(on);
  if (!m) return;
  uint32_t base = 0u;
  if (lane == (uint32_t)__ffsll((long long)m) - 1u) {
    base = atomicAdd(&J.ctl->open, (uint32_t)__popcll(m));
    atomicAdd(&J.ctl->contributing, (uint32_t)__popcll(m));
  }
  base = __shfl(base, __ffsll((long long)m) - 1);
  if (on) J.list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
}

// one wave per OPEN robot: lane g tries delay cur + g, then cur + 64 + g, ...
__global__ __launch_bounds__(kScheduleBlock) void k_schedule_probe(Job J)
{
  uint32_t open, round;
  if (!schedule_active(J, &open, &round)) return;
  const uint32_t W = blockIdx.x * (kScheduleBlock / 64) + (threadIdx.x >> 6), g = threadIdx.x & 63u, last = J.V - 1u;
  if (W >= open) return;                                              // (the whole wave)
  const uint32_t i = J.list[(size_t)(round & 1u) * J.n + W];
  const Lane L = schedule_lane(J, i);
  const bool light = L.w <= J.capacity;
  const uint32_t room = light ? J.capacity - L.w : 0u;                 // a constrained cell may hold this much before the robot
  uint32_t base = J.cur[i], found = mnav::kNone;
  for (;;) {
    const uint32_t d = base + g;
    const bool live = light && d <= J.max_delay;
    const float dep = schedule_depart(L.depart, d <= J.max_delay ? d : J.max_delay, J.tau);
    bool fit = live, beyond = false;
    uint32_t u = L.u;
    for (uint32_t q = 0; q <= L.len; ++q) {
      const float du = L.dist[u];
      const uint32_t p = L.pred[u];                                   // (of the seed too: never followed)
      uint32_t k = 0u;
      const bool in = timed_slot(timed_time(L.P, du, dep, L.pace), J.tau, J.B, &k);
      const uint32_t have = J.cell[(size_t)u * J.B + (in ? k : 0u)];  // unconditional, at a clamped window
      const bool constrained = !((J.flags & kSeedFree) && q == L.len);
      beyond = beyond || !in;
      fit = fit && in && !(constrained && have > room);
      if (!__ballot(fit)) break;
      u = p < last ? p : last;                                        // (fleet_classify has walked this chain: every id is a vertex)
    }
    const unsigned long long fits = __ballot(fit);
    if (fits) { found = base + (uint32_t)__ffsll((long long)fits) - 1u; break; }
    if (!light || __ballot(live && beyond) || base + 64u > J.max_delay) break;   // beyond the horizon: every larger delay is too
    base += 64u;
  }
  if (g == 0u) {
    if (found != mnav::kNone) J.cur[i] = found;
    else { J.st[i] = kStNoSlot; atomicAdd(&J.ctl->pend_no_slot, 1u); }
  }
}

// the OPEN robot of this lane (kNone: none) in a one-lane-per-robot pass
__device__ __forceinline__ uint32_t schedule_robot(const Job& J, uint32_t open, uint32_t round)
{
  const uint32_t t = blockIdx.x * kScheduleBlock + threadIdx.x;
  const uint32_t i = J.list[(size_t)(round & 1u) * J.n + (t < open ? t : open - 1u)];   // clamped: open >= 1
  return t < open && J.st[i] == kStOpen ? i : mnav::kNone;           // (the probe may just have given it NO_SLOT)
}

__global__ __launch_bounds__(kScheduleBlock) void k_schedule_claim(Job J)
{
  uint32_t open, round;
  if (!schedule_active(J, &open, &round)) return;
  const uint32_t i = schedule_robot(J, open, round), last = J.V - 1u;
  const unsigned long long act = __ballot(i != mnav::kNone);
  if (!act) return;
  if (i != mnav::kNone) {
    const Lane L = schedule_lane(J, i);
    const float dep = schedule_depart(L.depart, J.cur[i], J.tau);
    const unsigned long long ticket = schedule_ticket(L.key, i);
    uint32_t u = L.u;
    for (uint32_t q = 0; q <= L.len; ++q) {
      const float du = L.dist[u];
      const uint32_t p = L.pred[u];
      uint32_t k = 0u;
      const bool in = timed_slot(timed_time(L.P, du, dep, L.pace), J.tau, J.B, &k);   // (the probe saw every visit inside)
      if (in && !((J.flags & kSeedFree) && q == L.len)) {
        const size_t c = (size_t)u * J.B + k;
        atomicAdd(J.tent + c, L.w);
        atomicMin(J.thold + c, ticket);
      }
      u = p < last ? p : last;
    }
  }
  if ((threadIdx.x & 63u) == (uint32_t)__ffsll((long long)act) - 1u) atomicAdd(&J.ctl->claims, (unsigned long long)__popcll(act));
}

__global__ __launch_bounds__(kScheduleBlock) void k_schedule_decide(Job J)
{
  uint32_t open, round;
  if (!schedule_active(J, &open, &round)) return;
  const uint32_t i = schedule_robot(J, open, round), last = J.V - 1u;
  if (i == mnav::kNone) return;
  const Lane L = schedule_lane(J, i);
  const float dep = schedule_depart(L.depart, J.cur[i], J.tau);
  const unsigned long long ticket = schedule_ticket(L.key, i);
  uint32_t u = L.u, win = 1u;
  for (uint32_t q = 0; q <= L.len; ++q) {
    const float du = L.dist[u];
    const uint32_t p = L.pred[u];
    uint32_t k = 0u;
    const bool in = timed_slot(timed_time(L.P, du, dep, L.pace), J.tau, J.B, &k);
    const size_t c = (size_t)u * J.B + (in ? k : 0u);
    const unsigned long long all = (unsigned long long)J.cell[c] + J.tent[c];
    const unsigned long long holder = J.thold[c];
    if (in && !((J.flags & kSeedFree) && q == L.len) && all > J.capacity && holder != ticket) win = 0u;
    u = p < last ? p : last;
  }
  J.win[i] = win;
}

__global__ __launch_bounds__(kScheduleBlock) void k_schedule_commit(Job J)
{
  uint32_t open, round;
  if (!schedule_active(J, &open, &round)) return;
  const uint32_t i = schedule_robot(J, open, round), last = J.V - 1u, lane = threadIdx.x & 63u;
  const unsigned long long act = __ballot(i != mnav::kNone);
  if (!act) return;
  uint32_t win = 0u, w = 0u, visits = 0u, d = 0u;
  if (i != mnav::kNone) {
    const Lane L = schedule_lane(J, i);
    d = J.cur[i]; win = J.win[i];
    const float dep = schedule_depart(L.depart, d, J.tau);
    uint32_t u = L.u;
    for (uint32_t q = 0; q <= L.len; ++q) {
      const float du = L.dist[u];
      const uint32_t p = L.pred[u];
      uint32_t k = 0u;
      if (timed_slot(timed_time(L.P, du, dep, L.pace), J.tau, J.B, &k)) {
        const size_t c = (size_t)u * J.B + k;
        if (win) { atomicAdd(J.cell + c, L.w); atomicMin(J.holder + c, L.key); }
        if (J.undo && !((J.flags & kSeedFree) && q == L.len)) { J.tent[c] = 0u; J.thold[c] = kNoTicket; }   // (every claimant of the cell stores the same clean words)
      }
      u = p < last ? p : last;
    }
    if (win) {
      J.st[i] = kStCommitted; J.delay_out[i] = d; J.round_out[i] = round + 1u; J.depart_out[i] = dep;
      w = L.w; visits = L.len + 1u;
    }
  }
  // the round's counters: one atomic per wave and counter
  const unsigned long long won = __ballot(win != 0u), lost = act & ~won;
  const unsigned long long sum_w = mnav_traffic::wave_sum64(w), sum_v = mnav_traffic::wave_sum64(visits);
  const uint32_t late = (uint32_t)__popcll(__ballot(win != 0u && d > 0u));
  uint32_t dmax = win ? d : 0u;
  for (int o = 32; o > 0; o >>= 1) { const uint32_t y = __shfl_xor(dmax, o); dmax = y > dmax ? y : dmax; }
  const uint32_t lead = (uint32_t)__ffsll((long long)act) - 1u;
  uint32_t base = 0u;
  if (lane == lead) {
    if (won) {
      atomicAdd(&J.ctl->pend_won, (uint32_t)__popcll(won));
      atomicAdd(&J.ctl->visits, sum_v);
      atomicAdd(&J.ctl->weight, sum_w);
      if (late) atomicAdd(&J.ctl->delayed, late);
      atomicMax(&J.ctl->max_delay_used, dmax);
    }
    if (lost) base = atomicAdd(&J.ctl->pend_next, (uint32_t)__popcll(lost));
  }
  base = __shfl(base, (int)lead);
  if ((lost >> lane) & 1ull) J.list[(size_t)((round + 1u) & 1u) * J.n + base + (uint32_t)__popcll(lost & ((1ull << lane) - 1ull))] = i;   // OPEN again next round
}

// one lane: the round is over
__global__ void k_schedule_next(Job J)
{
  uint32_t open, round;
  if (!schedule_active(J, &open, &round)) return;
  Counts* K = J.ctl;
  K->committed += K->pend_won; K->no_slot += K->pend_no_slot;
  K->open = K->pend_next; K->round = round + 1u;
  K->pend_won = K->pend_no_slot = K->pend_next = 0u;
}

// the scratch and the statistics of the last mnav_fleet_schedule; dropped by mnav_upload_mesh
struct State {
  mnav::DevBuf<uint32_t> tent; mnav::DevBuf<unsigned long long> thold; size_t cells = 0; bool dirty = false;   // V x B each; dirty: not clean (the fill mode leaves the last round's claims)
  mnav::DevBuf<Counts> ctl;
  mnav::DevBuf<uint32_t> list, st, cur, win, delay, round; mnav::DevBuf<float> depart_out; size_t cap = 0;   // per robot (list: 2 per robot)
  Counts last = {}; uint32_t built_index = 0; float ms_kernels = 0.f, ms_total = 0.f;
};

#endif  // __HIPCC__

}  // namespace mnav_schedule
