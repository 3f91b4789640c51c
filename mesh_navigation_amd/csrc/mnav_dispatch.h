// mnav_dispatch.h -- fleet dispatch (mnav_fleet_costs, mnav_fleet_assign): which goal does each robot go to?
// With K goal fields resident and R robots, the cost of robot i to reach the goal of column j is one float, d_j[v_i],
// behind the O(1) head of the rule of mnav_fleet_paths (mnav_fleet.h).  The pair rule, first match
// wins; d / p = the column's resident dist / pred, g = its seed, t = its target, cut = goal_cut(d[t], offset, t).cut:
//   1  v >= V                              INVALID_GOAL
//   2  the plan never reached the device   the plan's own code
//   3  v == g                              SUCCESS, potential 0
//   4  d[v] < cut, or v == t               p[v] == v: NO_PATH_FOUND; else SUCCESS, potential d[v].  The chain is NOT walked:
//                                          a chain that does not reach g (INTERNAL_ERROR in mnav_fleet_paths) is not detected
//   5  d[v] == +inf and the wave ran out    NO_PATH_FOUND (lazily, as in mnav_fleet.h: k_fleet_open over the marked columns)
//   6  otherwise                           BEYOND_FIELD
// potential = +inf wherever rules 3 and 4 do not set it.  A pair is FEASIBLE when its code is SUCCESS and its potential is
// finite (that leaves out the seed == target plans of rule 2).  dispatch_pair is the device's own source and the host
// mirror's (tests/test_dispatch_model.py).
//
// Matrix pass, k_dispatch_costs: one workgroup of 4 waves per tile of 64 robots x 64 columns, robot tiles fastest in the
// grid: the intent is that the workgroups in flight share columns, not rows, so that the caches see few fields (dist and
// pred: 8 bytes x V per column) at a time; what that buys is in DESIGN.md section 3.15 (the achieved gather rate).  First half: lane =
// robot, wave w takes the columns w, w + 4, ... of the tile; the column's record is wave-uniform, dist and pred are
// gathered unconditionally at the clamped vertex through GPtr (no flat load), the pair goes into an LDS tile and a wave
// reduction over the 64 robots gives the column's minimum in this tile.  Second half: lane = column, wave w stores the
// rows w, w + 4, ... of the tile -- 256 contiguous bytes of potentials and 64 of codes per row -- and a wave reduction over
// the 64 columns gives the row's minimum in this tile.  Minima are 64-bit keys (potential bits, index): the smallest key is
// the smallest potential with ties to the smallest index; k_dispatch_nearest takes the minimum of a row's / column's tile
// keys, so no result depends on the order of atomics (the only atomics are integer sums of counters).
//
// Assignment: maximum size, then minimum sum of q = floor(potential / quantum + 0.5), by a synchronous (Jacobi) auction
// with eps-scaling on the padded N x N problem, N = max(n, m) -- the rule is spelled out at dispatch_auction_host below and
// in DESIGN.md section 3.15.  All arithmetic is int64.  One round = every unassigned bidder bids, every column takes its
// highest bid.  Wide rounds: k_dispatch_bid (one wave per bidder, lanes strided over the columns) + k_dispatch_award (one
// workgroup: winners, evictions, prices, the count, the phase).  Tail rounds: k_dispatch_tail, ONE workgroup that loops
// whole rounds with __syncthreads between the halves while at most `tail` bidders are unassigned.  Both run the same
// device functions on the same state, the mode of the next round is decided on the device, and a launch that finds
// the other mode (or the end) returns at once: the host launches rounds in chunks and reads one control record per
// chunk.  No kernel waits for another workgroup.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "mnav_fleet.h"

namespace mnav_dispatch {

using mnav::GPtr;
using mnav::kNone;
using mnav_fleet::Field;
using mnav_fleet::kBeyond;
using mnav_fleet::kInvalidGoal;
using mnav_fleet::kNoPath;
using mnav_fleet::kSuccess;

constexpr int kTile = 64;                 // robots and columns per tile of the matrix pass
constexpr int kDispBlock = 256;               // threads of the matrix pass and of the element-wise passes
constexpr int kCounters = 6;              // served, beyond field, no path, invalid, feasible, marked for rule 5 under a finite cut
constexpr uint32_t kPending = 0xFFu;      // code byte of a marked pair until k_dispatch_resolve has k_fleet_open's answer
constexpr unsigned long long kNoKey = ~0ull;
constexpr int32_t kInfeasible = -1;       // sentinel of the quantised matrix
constexpr long long kQMax = 0x7FFFFFFFll; // largest quantised cost
constexpr long long kMaxI64 = 0x7FFFFFFFFFFFFFFFll;
constexpr long long kBidLimit = 1ll << 62;
constexpr int kAuctionBlock = 1024;       // threads of k_dispatch_award and k_dispatch_tail
constexpr uint32_t kTailMax = 8192;       // bidders the tail kernel can list in LDS (32 KiB)
constexpr uint32_t kTailDefault = 16;     // default of the option dispatch_tail_bidders (measured: DESIGN.md section 3.15)
constexpr uint32_t kModeWide = 0u, kModeTail = 1u;
constexpr uint32_t kFlagDone = 1u, kFlagCapped = 2u, kFlagOverflow = 4u;

struct Pair { uint32_t code; float potential; bool unreached; };   // unreached: rule 5 or 6 under a finite cut (fleet_open_value decides)

// the pair rule on loaded values: d = dist[min(v, V - 1)], pv = pred[min(v, V - 1)] of the column (anything when it has no field)
MNAV_HD Pair dispatch_pair(const Field& Fd, uint32_t V, uint32_t v, float d, uint32_t pv)
{
  Pair R; R.code = kInvalidGoal; R.potential = mnav::inf_f(); R.unreached = false;
  if (v >= V) return R;                                               // rule 1
  if (!Fd.dist) { R.code = Fd.code; return R; }                       // rule 2
  if (v == Fd.seed) { R.code = kSuccess; R.potential = 0.f; return R; }   // rule 3
  if (d < Fd.cut || v == Fd.target) {                                 // rule 4, without the walk
    R.potential = d;
    R.code = pv == v ? kNoPath : kSuccess;
    return R;
  }
  R.code = (!(d < mnav::inf_f()) && !(Fd.cut < mnav::inf_f())) ? kNoPath : kBeyond;   // rules 5 and 6
  R.unreached = !(d < mnav::inf_f()) && Fd.cut < mnav::inf_f();
  return R;
}
MNAV_HD bool dispatch_feasible(uint32_t code, float potential) { return code == kSuccess && potential < mnav::inf_f(); }
// potentials are sums of non-negative edge weights: their bit patterns order as they do
MNAV_HD unsigned long long dispatch_key(float potential, uint32_t index) { return ((unsigned long long)mnav::f2u(potential) << 32) | index; }
MNAV_HD uint32_t dispatch_key_index(unsigned long long key) { return key == kNoKey ? kNone : (uint32_t)key; }
// q of a feasible pair; kQMax + 1 for anything above kQMax
MNAV_HD long long dispatch_quantise(float potential, double quantum)
{
  const double x = floor((double)potential / quantum + 0.5);
  return x <= (double)kQMax ? (long long)x : kQMax + 1;
}

// ---- the auction ----------------------------------------------------------------------------------------------------------
// Scaled cost of the padded pair (i, j): q (N + 1) for a feasible pair, M (N + 1) with M = N q_max + 1 for an infeasible
// real pair, 0 when i >= n or j >= m.
struct Control { long long eps; unsigned long long rounds, tail_rounds, bids; uint32_t unassigned, phases, mode, flags; };
struct Auction {
  uint32_t n, m, N, tail;
  const int32_t* q;                       // n x m, kInfeasible for an infeasible pair
  long long scale, big;                   // N + 1, M (N + 1)
  unsigned long long max_rounds;
  long long* price; uint32_t* owner; uint32_t* mine;        // per column: price, bidder; per bidder: column
  uint32_t* bidcol; long long* bidval;                      // per bidder: this round's bid
  unsigned long long* colbest; uint32_t* winner;            // per column: this round's highest bid and its smallest bidder
  Control* ctl;
};
struct Best { long long w1, w2; uint32_t j1; };   // smallest cost + price with its smallest column, and the smallest value over the other columns

MNAV_HD Best best_none() { Best b; b.w1 = kMaxI64; b.w2 = kMaxI64; b.j1 = kNone; return b; }
MNAV_HD void best_add(Best& b, long long w, uint32_t j)
{
  if (w < b.w1 || (w == b.w1 && j < b.j1)) { b.w2 = b.w1; b.w1 = w; b.j1 = j; }
  else if (w < b.w2) b.w2 = w;
}
MNAV_HD Best best_merge(Best a, Best b)   // associative and commutative
{
  const bool swap = b.w1 < a.w1 || (b.w1 == a.w1 && b.j1 < a.j1);
  Best lo = swap ? b : a; const Best hi = swap ? a : b;
  if (hi.w1 < lo.w2) lo.w2 = hi.w1;
  return lo;
}
MNAV_HD long long dispatch_cost(uint32_t n, uint32_t m, const int32_t* q, long long scale, long long big, uint32_t i, uint32_t j)
{
  if (i >= n || j >= m) return 0;
  const int32_t x = q[(size_t)i * m + j];
  return x < 0 ? big : (long long)x * scale;
}
// the price bidder offers for column b.j1: price + (second - best) + eps; a lone column has no second
MNAV_HD long long dispatch_bid(const Best& b, long long price, long long eps) { return price + (b.w2 == kMaxI64 ? 0 : b.w2 - b.w1) + eps; }
MNAV_HD long long dispatch_next_eps(long long eps) { return eps / 8 > 1 ? eps / 8 : 1; }

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host mirror ----------------------------------------------------------------------------------------------------------
// mnav_fleet_costs on host arrays: `cols` = the m columns' fields with host pointers and their cuts set.  code / potential:
// n x m; nearest_slot: n; nearest_robot: m; counters: served, beyond, no path, invalid, feasible.  Any output may be null.
inline void dispatch_costs_host(uint32_t n, uint32_t V, uint32_t m, const Field* cols, const uint32_t* vtx, uint8_t* code, float* potential,
                                uint32_t* nearest_slot, uint32_t* nearest_robot, unsigned long long* counters)
{
  std::vector<unsigned long long> row(n, kNoKey);
  for (uint32_t j = 0; j < m; ++j) {
    const Field& Fd = cols[j];
    int open = -1;                                                    // rule 5 under a finite cut: looked at when the first pair asks
    unsigned long long best = kNoKey;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t v = vtx[i], vc = v < V ? v : V - 1u;
      Pair R = dispatch_pair(Fd, V, v, Fd.dist ? Fd.dist[vc] : mnav::inf_f(), Fd.dist ? Fd.pred[vc] : 0u);
      if (R.unreached) {
        if (open < 0) { open = 0; for (uint32_t u = 0; u < V && !open; ++u) open = mnav_fleet::fleet_open_value(Fd.dist[u], Fd.cut) ? 1 : 0; }
        if (!open) R.code = kNoPath;
      }
      const size_t e = (size_t)i * m + j;
      if (code) code[e] = (uint8_t)R.code;
      if (potential) potential[e] = R.potential;
      const bool ok = dispatch_feasible(R.code, R.potential);
      if (counters) { counters[mnav_fleet::fleet_outcome(R.code)] += 1u; if (ok) counters[4] += 1u; }
      if (!ok) continue;
      if (dispatch_key(R.potential, i) < best) best = dispatch_key(R.potential, i);
      if (dispatch_key(R.potential, j) < row[i]) row[i] = dispatch_key(R.potential, j);
    }
    if (nearest_robot) nearest_robot[j] = dispatch_key_index(best);
  }
  for (uint32_t i = 0; nearest_slot && i < n; ++i) nearest_slot[i] = dispatch_key_index(row[i]);
}
// q (n x m, kInfeasible where infeasible) of a matrix; returns q_max, or kQMax + 1 when a cost is above kQMax
inline long long dispatch_quantise_host(size_t pairs, const uint8_t* code, const float* potential, double quantum, int32_t* q)
{
  long long qmax = 0;
  for (size_t e = 0; e < pairs; ++e) {
    q[e] = kInfeasible;
    if (!dispatch_feasible(code[e], potential[e])) continue;
    const long long x = dispatch_quantise(potential[e], quantum);
    if (x > qmax) qmax = x;
    q[e] = x > kQMax ? kInfeasible : (int32_t)x;
  }
  return qmax;
}
// The synchronous auction as the device runs it.  mine: N entries (bidder -> column of the padded problem).  Returns 0, or
// the flag that stopped it (kFlagCapped, kFlagOverflow).  The caller has checked (N + 1) (N q_max + 1) < 2^56.
//   eps = max(1, C / 2), C = the largest scaled cost; prices 0, nobody assigned
//   round: every unassigned bidder i takes w_j = cost(i, j) + price_j over all N columns, its best column j1 (smallest w,
//          ties to the smallest j) and the smallest w over the other columns, and bids dispatch_bid for j1; then every
//          column with bids takes the highest (ties to the smallest bidder) as its price and owner; the old owner is
//          unassigned again
//   when nobody is unassigned: done if eps == 1; else eps = max(1, eps / 8), everybody unassigned, prices kept
inline uint32_t dispatch_auction_host(uint32_t n, uint32_t m, const int32_t* q, long long qmax, bool any_infeasible, unsigned long long max_rounds, uint32_t* mine,
                                      uint32_t* phases, unsigned long long* rounds, unsigned long long* bids)
{
  const uint32_t N = n > m ? n : m;
  const long long scale = (long long)N + 1, big = ((long long)N * qmax + 1) * scale;
  const long long C = any_infeasible ? big : qmax * scale;
  long long eps = C / 2 > 1 ? C / 2 : 1;
  std::vector<long long> price(N, 0), bidval(N, 0);
  std::vector<uint32_t> owner(N, kNone), bidcol(N, kNone);
  for (uint32_t i = 0; i < N; ++i) mine[i] = kNone;
  uint32_t unassigned = N;
  *phases = 1; *rounds = 0; *bids = 0;
  for (;;) {
    for (uint32_t i = 0; i < N; ++i) {
      bidcol[i] = kNone;
      if (mine[i] != kNone) continue;
      Best b = best_none();
      for (uint32_t j = 0; j < N; ++j) best_add(b, dispatch_cost(n, m, q, scale, big, i, j) + price[j], j);
      bidcol[i] = b.j1; bidval[i] = dispatch_bid(b, price[b.j1], eps);
      if (bidval[i] >= kBidLimit) return kFlagOverflow;
    }
    *bids += unassigned;
    for (uint32_t j = 0; j < N; ++j) {
      uint32_t win = kNone;
      for (uint32_t i = 0; i < N; ++i) if (bidcol[i] == j && (win == kNone || bidval[i] > bidval[win])) win = i;
      if (win == kNone) continue;
      if (owner[j] != kNone) mine[owner[j]] = kNone; else --unassigned;
      owner[j] = win; mine[win] = j; price[j] = bidval[win];
    }
    *rounds += 1;
    if (!unassigned) {
      if (eps == 1) return 0;
      eps = dispatch_next_eps(eps); *phases += 1; unassigned = N;
      for (uint32_t i = 0; i < N; ++i) { owner[i] = kNone; mine[i] = kNone; }
    }
    if (*rounds >= max_rounds) return kFlagCapped;
  }
}
#endif

#if defined(__HIPCC__)

struct Costs {
  uint32_t n, m, V;
  const uint32_t* vtx; const Field* cols;
  uint8_t* code; float* potential;
  unsigned long long* rowpart; unsigned long long* colpart;   // [column tile][robot], [robot tile][column]: the tile minima
  uint32_t* need; unsigned long long* cnt;                    // per column: waits for k_fleet_open; kCounters sums
};

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long k)
{
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long x = __shfl_xor(k, o, 64);
    k = x < k ? x : k;
  }
  return k;
}

// LDS: 64 x 65 floats + 64 x 68 bytes + 6 words = 21 016 bytes per workgroup
__global__ __launch_bounds__(kDispBlock) void k_dispatch_costs(Costs P)
{
  __shared__ float s_pot[kTile][kTile + 1];
  __shared__ uint8_t s_code[kTile][kTile + 4];
  __shared__ unsigned int s_cnt[kCounters];
  const uint32_t RT = (P.n + kTile - 1) / kTile;
  const uint32_t rt = blockIdx.x % RT, ct = blockIdx.x / RT;         // robot tiles fastest: neighbours in the grid share columns
  const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (threadIdx.x < (uint32_t)kCounters) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  {
    const uint32_t i = rt * kTile + lane;
    const bool robot = i < P.n;
    const uint32_t v = robot ? P.vtx[i] : kNone;
    const uint32_t vc = v < P.V ? v : P.V - 1u;
    uint32_t outcomes = 0u, extra = 0u;                               // 4 x 8 bits: pairs per outcome; 2 x 16 bits: feasible, marked (<= 16 columns per wave)
    for (uint32_t c = wave; c < (uint32_t)kTile; c += kDispBlock / 64) {
      const uint32_t j = ct * kTile + c;
      if (j >= P.m) break;                                            // wave-uniform
      const Field Fd = P.cols[j];
      float d = mnav::inf_f(); uint32_t pv = 0u;
      if (Fd.dist) { d = Fd.dist[vc]; pv = Fd.pred[vc]; }             // wave-uniform test; the loads do not wait for the rule
      const Pair R = dispatch_pair(Fd, P.V, v, d, pv);
      const bool ok = dispatch_feasible(R.code, R.potential);
      s_pot[lane][c] = R.potential;
      s_code[lane][c] = (uint8_t)(R.unreached ? kPending : R.code);
      const unsigned long long key = wave_min_u64(robot && ok ? dispatch_key(R.potential, i) : kNoKey);
      const unsigned long long marked = __ballot(R.unreached);
      if (lane == 0u) {
        P.colpart[(size_t)rt * P.m + j] = key;
        if (marked) P.need[j] = 1u;
      }
      if (robot) { outcomes += 1u << (8 * mnav_fleet::fleet_outcome(R.code)); extra += (ok ? 1u : 0u) + (R.unreached ? 0x10000u : 0u); }
    }
    for (int k = 0; k < 4; ++k) if ((outcomes >> (8 * k)) & 0xFFu) atomicAdd(&s_cnt[k], (outcomes >> (8 * k)) & 0xFFu);
    if (extra & 0xFFFFu) atomicAdd(&s_cnt[4], extra & 0xFFFFu);
    if (extra >> 16) atomicAdd(&s_cnt[5], extra >> 16);
  }
  __syncthreads();
  const uint32_t j = ct * kTile + lane;
  for (uint32_t r = wave; r < (uint32_t)kTile; r += kDispBlock / 64) {
    const uint32_t i = rt * kTile + r;
    if (i >= P.n) break;                                              // wave-uniform
    unsigned long long key = kNoKey;
    if (j < P.m) {
      const float pot = s_pot[r][lane];
      const uint32_t code = s_code[r][lane];
      const size_t e = (size_t)i * P.m + j;
      P.potential[e] = pot; P.code[e] = (uint8_t)code;               // whole lines: 64 consecutive floats / bytes of one row
      if (dispatch_feasible(code, pot)) key = dispatch_key(pot, j);
    }
    key = wave_min_u64(key);
    if (lane == 0u) P.rowpart[(size_t)ct * P.n + i] = key;
  }
  if (threadIdx.x < (uint32_t)kCounters && s_cnt[threadIdx.x]) atomicAdd(P.cnt + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

// the marked pairs once k_fleet_open has looked: BEYOND_FIELD where the column holds a finite value at or above its cut, NO_PATH_FOUND elsewhere
__global__ __launch_bounds__(kDispBlock) void k_dispatch_resolve(unsigned long long pairs, uint32_t m, uint8_t* __restrict__ code, const uint32_t* __restrict__ open,
                                                            unsigned long long* __restrict__ cnt)
{
  uint32_t moved = 0u;
  for (unsigned long long e = (unsigned long long)blockIdx.x * kDispBlock + threadIdx.x; e < pairs; e += (unsigned long long)gridDim.x * kDispBlock) {
    if (code[e] != kPending) continue;
    const bool is_open = open[(uint32_t)(e % m)] != 0u;
    code[e] = (uint8_t)(is_open ? kBeyond : kNoPath);
    moved += is_open ? 0u : 1u;
  }
  for (int o = 32; o > 0; o >>= 1) moved += __shfl_xor(moved, o, 64);
  if ((threadIdx.x & 63u) == 0u && moved) {
    atomicAdd(cnt + 1, (unsigned long long)(0ll - (long long)moved));   // counted as beyond the field by the matrix pass
    atomicAdd(cnt + 2, (unsigned long long)moved);
  }
}

// thread t < n: robot t over its column tiles; n <= t < n + m: column t - n over its robot tiles
__global__ __launch_bounds__(kDispBlock) void k_dispatch_nearest(uint32_t n, uint32_t m, const unsigned long long* __restrict__ rowpart,
                                                            const unsigned long long* __restrict__ colpart, uint32_t* __restrict__ nearest_slot,
                                                            uint32_t* __restrict__ nearest_robot)
{
  const uint32_t t = blockIdx.x * kDispBlock + threadIdx.x;
  const uint32_t RT = (n + kTile - 1) / kTile, CT = (m + kTile - 1) / kTile;
  unsigned long long key = kNoKey;
  if (t < n) {
    for (uint32_t c = 0; c < CT; ++c) { const unsigned long long k = rowpart[(size_t)c * n + t]; key = k < key ? k : key; }
    nearest_slot[t] = dispatch_key_index(key);
  } else if (t - n < m) {
    const uint32_t j = t - n;
    for (uint32_t r = 0; r < RT; ++r) { const unsigned long long k = colpart[(size_t)r * m + j]; key = k < key ? k : key; }
    nearest_robot[j] = dispatch_key_index(key);
  }
}

// info[0] = q_max (atomicMax: the result does not depend on the order), info[1] |= 1 when a cost is above kQMax
__global__ __launch_bounds__(kDispBlock) void k_dispatch_quantise(unsigned long long pairs, const uint8_t* __restrict__ code, const float* __restrict__ potential,
                                                             double quantum, int32_t* __restrict__ q, uint32_t* __restrict__ info)
{
  uint32_t qmax = 0u, big = 0u;
  for (unsigned long long e = (unsigned long long)blockIdx.x * kDispBlock + threadIdx.x; e < pairs; e += (unsigned long long)gridDim.x * kDispBlock) {
    int32_t out = kInfeasible;
    const float pot = potential[e];
    if (dispatch_feasible(code[e], pot)) {
      const long long x = dispatch_quantise(pot, quantum);
      if (x > kQMax) big = 1u; else { out = (int32_t)x; qmax = (uint32_t)x > qmax ? (uint32_t)x : qmax; }
    }
    q[e] = out;
  }
  for (int o = 32; o > 0; o >>= 1) { const uint32_t x = __shfl_xor(qmax, o, 64); qmax = x > qmax ? x : qmax; }
  const unsigned long long any_big = __ballot(big != 0u);
  if ((threadIdx.x & 63u) == 0u) {
    if (qmax) atomicMax(info, qmax);
    if (any_big) atomicOr(info + 1, 1u);
  }
}

// The auction's state is read and written at device scope in the tail kernel and in the award pass: the tail kernel reads
// in one round what another wave of its workgroup wrote in the round before.  The wide bid kernel reads the prices with
// plain loads (Wide): the kernel boundary orders them after the award pass that wrote them.
template <class T> __device__ __forceinline__ T ld(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class T> __device__ __forceinline__ void st(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ Best wave_best(Best b)
{
  for (int o = 32; o > 0; o >>= 1) {
    Best x;
    x.w1 = __shfl_xor(b.w1, o, 64); x.w2 = __shfl_xor(b.w2, o, 64); x.j1 = __shfl_xor(b.j1, o, 64);
    b = best_merge(b, x);
  }
  return b;
}

// one wave: the bid of unassigned bidder i
template <bool Wide> __device__ __forceinline__ void dispatch_bid_wave(const Auction& A, uint32_t i, uint32_t lane, long long eps)
{
  Best b = best_none();
  for (uint32_t j = lane; j < A.N; j += 64u) best_add(b, dispatch_cost(A.n, A.m, A.q, A.scale, A.big, i, j) + (Wide ? A.price[j] : ld(A.price + j)), j);
  b = wave_best(b);
  if (lane == 0u) {
    const long long bid = dispatch_bid(b, Wide ? A.price[b.j1] : ld(A.price + b.j1), eps);
    st(A.bidcol + i, b.j1); st(A.bidval + i, bid);
    atomicMax(A.colbest + b.j1, (unsigned long long)bid);           // the maximum does not depend on the order
    if (bid >= kBidLimit) atomicOr(&A.ctl->flags, kFlagOverflow);
  }
}

// Every thread of ONE workgroup, after all bids of the round: winners (the smallest bidder among a column's highest bids),
// evictions, prices, the count of unassigned bidders, the end of the phase and the mode of the next round.
__device__ __forceinline__ void dispatch_award_block(const Auction& A, bool tail, uint32_t* s_word)
{
  const uint32_t t = threadIdx.x, nt = blockDim.x;
  if (t == 0u) { s_word[0] = 0u; s_word[1] = 0u; }
  for (uint32_t i = t; i < A.N; i += nt) {
    const uint32_t j = ld(A.bidcol + i);
    if (j != kNone && (unsigned long long)ld(A.bidval + i) == ld(A.colbest + j)) atomicMin(A.winner + j, i);
  }
  __syncthreads();
  uint32_t newly = 0u;                                                // columns without an owner that got one
  for (uint32_t j = t; j < A.N; j += nt) {
    const uint32_t w = ld(A.winner + j);
    if (w == kNone) continue;
    const uint32_t old = ld(A.owner + j);
    if (old != kNone) st(A.mine + old, kNone); else ++newly;          // (old did not bid in this round, w owns no column: no two threads meet)
    st(A.owner + j, w); st(A.mine + w, j);
    st(A.price + j, (long long)ld(A.colbest + j));
    st(A.winner + j, kNone); st(A.colbest + j, 0ull);
  }
  if (newly) atomicAdd(&s_word[0], newly);
  __syncthreads();
  if (t == 0u) {
    Control c;
    c.eps = ld(&A.ctl->eps); c.rounds = ld(&A.ctl->rounds); c.tail_rounds = ld(&A.ctl->tail_rounds); c.bids = ld(&A.ctl->bids);
    c.unassigned = ld(&A.ctl->unassigned); c.phases = ld(&A.ctl->phases); c.flags = 0u;
    c.bids += c.unassigned;
    c.unassigned -= s_word[0];
    c.rounds += 1ull;
    if (tail) c.tail_rounds += 1ull;
    if (!c.unassigned) {
      if (c.eps == 1) c.flags |= kFlagDone;
      else { c.eps = dispatch_next_eps(c.eps); c.phases += 1u; c.unassigned = A.N; s_word[1] = 1u; }
    }
    if (!(c.flags & kFlagDone) && c.rounds >= A.max_rounds) c.flags |= kFlagCapped;
    c.mode = c.unassigned <= A.tail ? kModeTail : kModeWide;
    st(&A.ctl->eps, c.eps); st(&A.ctl->rounds, c.rounds); st(&A.ctl->tail_rounds, c.tail_rounds); st(&A.ctl->bids, c.bids);
    st(&A.ctl->unassigned, c.unassigned); st(&A.ctl->phases, c.phases); st(&A.ctl->mode, c.mode);
    if (c.flags) atomicOr(&A.ctl->flags, c.flags);
  }
  __syncthreads();
  if (s_word[1]) for (uint32_t j = t; j < A.N; j += nt) { st(A.owner + j, kNone); st(A.mine + j, kNone); }   // a new phase: prices stay
  __syncthreads();
}

// a wide round, first half: one wave per bidder of the padded problem
__global__ __launch_bounds__(kDispBlock) void k_dispatch_bid(Auction A)
{
  const uint32_t i = blockIdx.x * (kDispBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (i >= A.N || ld(&A.ctl->flags) || ld(&A.ctl->mode) != kModeWide) return;
  if (ld(A.mine + i) != kNone) { if (lane == 0u) st(A.bidcol + i, kNone); return; }
  dispatch_bid_wave<true>(A, i, lane, ld(&A.ctl->eps));
}
// a wide round, second half: one workgroup
__global__ __launch_bounds__(kAuctionBlock) void k_dispatch_award(Auction A)
{
  __shared__ uint32_t s_word[2];
  if (ld(&A.ctl->flags) || ld(&A.ctl->mode) != kModeWide) return;     // (the same for every thread: nobody has written since the launch)
  dispatch_award_block(A, false, s_word);
}
// up to `budget` whole rounds in ONE workgroup, while the mode is the tail's
__global__ __launch_bounds__(kAuctionBlock) void k_dispatch_tail(Auction A, uint32_t budget)
{
  __shared__ uint32_t s_word[2];
  __shared__ uint32_t s_count;
  __shared__ uint32_t s_list[kTailMax];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  for (uint32_t r = 0; r < budget; ++r) {
    if (ld(&A.ctl->flags) || ld(&A.ctl->mode) != kModeTail) return;   // (written by thread 0 before the last barrier of the round before)
    const long long eps = ld(&A.ctl->eps);
    if (t == 0u) s_count = 0u;
    __syncthreads();
    for (uint32_t i = t; i < A.N; i += kAuctionBlock) {
      if (ld(A.mine + i) != kNone) { st(A.bidcol + i, kNone); continue; }
      const uint32_t k = atomicAdd(&s_count, 1u);                     // (the order of the list decides nothing)
      if (k < kTailMax) s_list[k] = i;
    }
    __syncthreads();
    const uint32_t count = s_count < kTailMax ? s_count : kTailMax;   // (mode == tail: unassigned <= tail <= kTailMax)
    for (uint32_t k = wave; k < count; k += kAuctionBlock / 64) dispatch_bid_wave<false>(A, s_list[k], lane, eps);
    __syncthreads();
    dispatch_award_block(A, true, s_word);
  }
}

// per robot: the column it holds when that pair is feasible
__global__ __launch_bounds__(kDispBlock) void k_dispatch_result(Auction A, const float* __restrict__ potential, const uint32_t* __restrict__ col_slot,
                                                           uint32_t* __restrict__ col_out, uint32_t* __restrict__ slot_out, float* __restrict__ pot_out,
                                                           int32_t* __restrict__ q_out)
{
  const uint32_t i = blockIdx.x * kDispBlock + threadIdx.x;
  if (i >= A.n) return;
  const uint32_t j = A.mine[i];
  const bool real = j < A.m;
  const size_t e = (size_t)i * A.m + (real ? j : 0u);
  const int32_t q = real ? A.q[e] : kInfeasible;
  const bool ok = q >= 0;
  col_out[i] = ok ? j : kNone; slot_out[i] = ok ? col_slot[j] : kNone;
  pot_out[i] = ok ? potential[e] : mnav::inf_f(); q_out[i] = ok ? q : kInfeasible;
}

// statistics of the last successful dispatch call
struct Stats {
  unsigned long long pairs[4] = { 0, 0, 0, 0 }, feasible = 0, rounds = 0, tail_rounds = 0, bids = 0;
  uint32_t assigned = 0, phases = 0, built_index = 0; float ms_costs = 0.f, ms_assign = 0.f, ms_total = 0.f;
};
struct State {
  mnav::DevBuf<uint32_t> vtx; size_t robots_cap = 0;
  mnav::DevBuf<Field> cols; mnav::DevBuf<uint32_t> need, col_slot; size_t cols_cap = 0;        // need: a word per column, then k_fleet_open's answers
  mnav::DevBuf<uint8_t> code; mnav::DevBuf<float> potential; size_t pairs_cap = 0;
  mnav::DevBuf<unsigned long long> rowpart, colpart, cnt;
  mnav::DevBuf<uint32_t> nearest; size_t nearest_cap = 0;                                     // n robots, then m columns
  mnav::DevBuf<int32_t> q; size_t q_cap = 0;
  mnav::DevBuf<long long> price, bidval; mnav::DevBuf<unsigned long long> colbest; mnav::DevBuf<uint32_t> words; size_t auction_cap = 0;   // words: owner, mine, bidcol, winner
  mnav::DevBuf<uint32_t> result; size_t result_cap = 0;                                       // per robot: column, slot, potential bits, q
  mnav::DevBuf<Control> ctl; mnav::DevBuf<uint32_t> info;
  mnav::Event ev[2]; bool have_ev = false;
  Stats stats;
};

#endif  // __HIPCC__

}  // namespace mnav_dispatch
