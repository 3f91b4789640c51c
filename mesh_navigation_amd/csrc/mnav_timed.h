// mnav_timed.h -- timed fleet traffic (mnav_fleet_timed_traffic, mnav_layer_timed_traffic, mnav_map_timed_traffic): how many
// planned paths cross each vertex IN EACH TIME WINDOW, who holds an over-full cell and who has to yield (DESIGN.md section
// 3.18).  The context owns V x B uint32 cells and V x B uint32 holders (row-major: cell[v * B + k]), the 64-bit total T of the
// accumulated weight, and per vertex the peak over its windows and the first window that attains it.
// A call carries B windows (1 .. 1024) of width tau.  Robot i contributes iff traffic_contributes (mnav_traffic.h) holds and
// w_i > 0.  A contributor on vertex v with potential P visits u = v, pred[v], ..., seed -- len + 1 visits -- and reaches u
// at (all float32, separate operations, no contraction)
//   dt = fmaxf(P - dist[u], 0.f);  t = depart_i + dt * pace_i;  q = t / (float)tau;  in the horizon iff q < (float)B;  k = (uint32_t)q
// An in-horizon visit adds w_i to cell[u][k] and lowers holder[u][k] (initially 0xFFFFFFFF) to min(holder, key_i); a visit
// beyond the horizon adds nothing and is counted.  Integer sums and minima do not depend on their order: cells and holders
// are the same bits on every schedule of the atomics, in one call or in several.
// The report runs after ALL adds of the call: a visit is OVER when cell[u][k] > free_count, and it YIELDS when it is over
// and holder[u][k] != key_i.  Robots with equal keys in one cell are both its holders: neither yields there.  With
// free_count > 0 every robot of an over cell but the holder yields, which is more than strictly must (free_count of them
// could stay); a loop that staggers the yielding robots still converges because every round counts again.
// timed_time / timed_slot / timed_window, timed_refusal and -- over fleet_classify -- timed_counts_host are the device's own
// source and the host mirror's (tests/test_timed_traffic_model.py).
//
// Device shape: classification and hop counts are k_fleet_cut / k_fleet_len (and k_fleet_open / _resolve for rule 5) of
// mnav_fleet.h, unchanged.  k_timed_add: one lane per robot walks its len + 1 visits -- the count is known, no walk is
// unbounded; per hop pred[u] and dist[u] are loaded together through GPtr (global loads) at the clamped index, then one
// no-return atomicAdd on the cell and one no-return atomicMin on the holder; the call's 64-bit sums are wave reductions with
// one atomic per wave.  k_timed_peak: a group of G = min(64, B rounded up to a power of two) lanes per vertex, lane g reads
// the windows g, g + G, ... of the vertex's contiguous row (consecutive lanes read consecutive words; one lane per vertex
// when B == 1), a shuffle reduction over the group gives the peak and the smallest window that attains it; a fixed number of
// blocks strides over the vertices, so the statistics of the cells cost one atomic per block.  k_timed_report:
// a launch after the adds (the kernel boundary orders the reads), the same walk with plain loads of cell and holder.  No
// kernel waits for another workgroup.
#pragma once
#include <cmath>
#include <cstdint>

#include "mnav_traffic.h"

namespace mnav_timed {

using mnav_fleet::Field;
using mnav_fleet::Robot;
using mnav_traffic::traffic_contributes;

constexpr int kTimedBlock = 256;                          // robots / lanes per block
constexpr uint32_t kMaxWindows = 1024u;
constexpr uint32_t kPeakBlocks = 2048u;                   // k_timed_peak: one block per 4 of the 8 192 waves an MI355X holds
constexpr unsigned long long kMaxTotal = mnav_traffic::kMaxTotal;   // T never exceeds it: no cell can wrap
// the 64-bit words of one call: sums of the adds, statistics of the cells, the yielding robots
enum { kContributing = 0, kAdds, kBeyond, kWeight, kOccupied, kOver, kLargest, kYielding, kWords };

// when a robot that left at `depart` and needs `pace` per unit of potential reaches a vertex of potential d_u on its way down from P
MNAV_HD float timed_time(float P, float d_u, float depart, float pace)
{
  const float dt = fmaxf(P - d_u, 0.f);
  const float along = dt * pace;
  return depart + along;
}
// the window of time t: false beyond the horizon (+inf included)
MNAV_HD bool timed_slot(float t, float tau, uint32_t B, uint32_t* k)
{
  const float q = t / tau;
  if (!(q < (float)B)) return false;
  *k = (uint32_t)q;                                                   // q >= 0: truncation
  return true;
}
MNAV_HD bool timed_window(float P, float d_u, float depart, float pace, float tau, uint32_t B, uint32_t* k)
{
  return timed_slot(timed_time(P, d_u, depart, pace), tau, B, k);
}

// What a call refuses before it touches anything, over ALL n robots (null: none).  state_B == 0: no cells yet.  Host code:
// the C ABI's check and the host mirror's.
inline const char* timed_refusal(uint32_t n, const uint32_t* weights, const float* depart, const float* pace, uint32_t B, double tau, int accumulate,
                                 unsigned long long T, uint32_t state_B, float state_tau)
{
  if (B < 1u || B > kMaxWindows) return "windows out of range (1 .. 1024)";
  const float tf = (float)tau;
  if (!std::isfinite(tf) || !(tf > 0.f)) return "tau must be finite and positive as a float";
  if (depart) for (uint32_t i = 0; i < n; ++i) if (!std::isfinite(depart[i]) || depart[i] < 0.f) return "a departure time is not finite or is negative";
  if (pace) for (uint32_t i = 0; i < n; ++i) if (!std::isfinite(pace[i]) || !(pace[i] > 0.f)) return "a pace is not finite or is not positive";
  if (accumulate && state_B && (state_B != B || state_tau != tf)) return "accumulate: windows or tau differ from the cells' configuration";
  unsigned long long all = accumulate ? T : 0ull;
  if (weights) for (uint32_t i = 0; i < n; ++i) all += weights[i];    // (n < 2^31 words of 32 bits: no 64-bit overflow)
  else all += n;
  if (all > kMaxTotal) return "total weight does not fit the counters";
  return nullptr;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// peak / first window per vertex and the statistics of the cells
inline void timed_peak_host(uint32_t V, uint32_t B, const uint32_t* cell, uint32_t free_count, uint32_t* peak, uint32_t* window, unsigned long long* words)
{
  words[kOccupied] = words[kOver] = words[kLargest] = 0ull;
  for (uint32_t v = 0; v < V; ++v) {
    uint32_t m = 0u, at = mnav::kNone;
    for (uint32_t k = 0; k < B; ++k) {
      const uint32_t x = cell[(size_t)v * B + k];
      if (x > m) { m = x; at = k; }
      words[kOccupied] += x > 0u; words[kOver] += x > free_count;
    }
    peak[v] = m; window[v] = at;
    if (m > words[kLargest]) words[kLargest] = m;
  }
}

// mnav_fleet_timed_traffic on host arrays: `fields` with host pointers and their cuts set; cell / holder (V x B words), *T,
// peak / window (V words) the context's state, whose configuration is (state_B, state_tau) when it has one.  Returns -1
// with nothing touched on a refusal.  Per robot (any may be null): code, potential, conflict, yield, fy_vertex, fy_window,
// fy_time; words: kWords (may be null).
inline int timed_counts_host(uint32_t n, uint32_t V, const Field* fields, const uint32_t* slot, const uint32_t* vtx, const uint32_t* weights, const float* depart,
                             const float* pace, const uint32_t* key, uint32_t B, double tau, uint32_t free_count, int accumulate, uint32_t state_B,
                             float state_tau, uint32_t* cell, uint32_t* holder, unsigned long long* T, uint32_t* peak, uint32_t* window, uint32_t* code,
                             float* potential, uint32_t* conflict, uint32_t* yield, uint32_t* fy_vertex, uint32_t* fy_window, float* fy_time,
                             unsigned long long* words)
{
  if (timed_refusal(n, weights, depart, pace, B, tau, accumulate, *T, state_B, state_tau)) return -1;
  const float tf = (float)tau;
  if (!accumulate) { for (size_t c = 0; c < (size_t)V * B; ++c) { cell[c] = 0u; holder[c] = mnav::kNone; } *T = 0ull; }
  unsigned long long s[kWords] = {};
  struct Seen { uint32_t len; float P; bool on; };
  Seen* seen = new Seen[n ? n : 1];
  for (uint32_t i = 0; i < n; ++i) {
    const Field& Fd = fields[slot[i]];
    Robot R = mnav_fleet::fleet_classify(Fd, V, vtx[i]);
    if (R.unreached) {                                                // rule 5 under a finite cut: did the wave run out?
      bool open = false;
      for (uint32_t u = 0; u < V && !open; ++u) open = mnav_fleet::fleet_open_value(Fd.dist[u], Fd.cut);
      if (!open) R.code = mnav_fleet::kNoPath;
    }
    if (code) code[i] = R.code;
    if (potential) potential[i] = R.potential;
    const uint32_t w = weights ? weights[i] : 1u;
    seen[i].len = R.len; seen[i].P = R.potential; seen[i].on = traffic_contributes(R.code, R.potential) && w;
    if (!seen[i].on) continue;
    const float dep = depart ? depart[i] : 0.f, pc = pace ? pace[i] : 1.f;
    const uint32_t ky = key ? key[i] : i;
    uint32_t u = vtx[i];
    for (uint32_t q = 0; q <= R.len; ++q) {                           // len + 1 visits, the last one on the seed
      uint32_t k;
      if (timed_window(R.potential, Fd.dist[u], dep, pc, tf, B, &k)) {
        const size_t c = (size_t)u * B + k;
        cell[c] += w; if (ky < holder[c]) holder[c] = ky;
        s[kAdds] += 1ull;
      } else s[kBeyond] += 1ull;
      u = Fd.pred[u];
    }
    s[kContributing] += 1ull; s[kWeight] += w;
  }
  *T += s[kWeight];
  timed_peak_host(V, B, cell, free_count, peak, window, s);
  // the report: on the cells as they stand after all adds
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t over = 0u, yl = 0u, fv = mnav::kNone, fw = mnav::kNone; float ft = mnav::inf_f();
    if (seen[i].on) {
      const Field& Fd = fields[slot[i]];
      const float dep = depart ? depart[i] : 0.f, pc = pace ? pace[i] : 1.f;
      const uint32_t ky = key ? key[i] : i;
      uint32_t u = vtx[i];
      for (uint32_t q = 0; q <= seen[i].len; ++q) {
        const float t = timed_time(seen[i].P, Fd.dist[u], dep, pc);
        uint32_t k;
        if (timed_slot(t, tf, B, &k)) {
          const size_t c = (size_t)u * B + k;
          if (cell[c] > free_count) {
            ++over;
            if (holder[c] != ky) { if (!yl) { fv = u; fw = k; ft = t; } ++yl; }
          }
        }
        u = Fd.pred[u];
      }
    }
    if (conflict) conflict[i] = over;
    if (yield) yield[i] = yl;
    if (fy_vertex) fy_vertex[i] = fv;
    if (fy_window) fy_window[i] = fw;
    if (fy_time) fy_time[i] = ft;
    s[kYielding] += yl > 0u;
  }
  delete[] seen;
  if (words) for (int k = 0; k < kWords; ++k) words[k] = s[k];
  return 0;
}
#endif

#if defined(__HIPCC__)

// the robots of one call as k_timed_add and k_timed_report see them
struct Walk {
  uint32_t n, V, B; float tau; uint32_t free_count;
  const uint32_t* slot; const uint32_t* vtx; const Field* fields;
  const uint32_t* code; const uint32_t* len; const float* potential;   // of k_fleet_len (a later k_fleet_resolve moves no MNAV_SUCCESS)
  const uint32_t* weight; const float* depart; const float* pace; const uint32_t* key;   // null: 1, 0, 1, the robot's index
  uint32_t* cell; uint32_t* holder; unsigned long long* words;
  uint32_t* conflict; uint32_t* yield; uint32_t* fy_vertex; uint32_t* fy_window; float* fy_time;   // the report, per robot
};

// One robot per lane, loaded unconditionally at the clamped index (n >= 1); visits == 0: the lane has nothing to walk.
struct Lane { uint32_t u, visits, w, key; float P, depart, pace; mnav::GPtr<const float> dist; mnav::GPtr<const uint32_t> pred; };
__device__ __forceinline__ Lane timed_lane(const Walk& A, uint32_t i)
{
  const uint32_t j = i < A.n ? i : A.n - 1u, last = A.V - 1u;
  const uint32_t s = A.slot[j], v = A.vtx[j], code = A.code[j], len = A.len[j];
  Lane L;
  L.P = A.potential[j];
  L.w = A.weight ? A.weight[j] : 1u;                                  // (wave-uniform branches)
  L.depart = A.depart ? A.depart[j] : 0.f;
  L.pace = A.pace ? A.pace[j] : 1.f;
  L.key = A.key ? A.key[j] : j;
  if (i >= A.n || !traffic_contributes(code, L.P)) L.w = 0u;
  L.dist = A.fields[s].dist; L.pred = A.fields[s].pred;
  L.visits = L.w ? len + 1u : 0u;
  L.u = v < last ? v : last;                                          // a contributor stands on a vertex (rule 1)
  return L;
}

__global__ __launch_bounds__(kTimedBlock) void k_timed_add(Walk A)
{
  const uint32_t i = blockIdx.x * kTimedBlock + threadIdx.x, last = A.V - 1u;
  const Lane L = timed_lane(A, i);
  uint32_t u = L.u, in = 0u;
  for (uint32_t q = 0; q < L.visits; ++q) {
    const float d = L.dist[u];
    const uint32_t p = L.pred[u];                                     // (of the seed too: never followed)
    uint32_t k;
    if (timed_window(L.P, d, L.depart, L.pace, A.tau, A.B, &k)) {
      const size_t c = (size_t)u * A.B + k;
      atomicAdd(A.cell + c, L.w);
      atomicMin(A.holder + c, L.key);
      ++in;
    }
    u = p < last ? p : last;                                          // (fleet_classify has walked this chain: every id is a vertex)
  }
  const unsigned long long act = __ballot(L.w != 0u);
  if (!act) return;
  const unsigned long long adds = mnav_traffic::wave_sum64(in), beyond = mnav_traffic::wave_sum64(L.visits - in), weight = mnav_traffic::wave_sum64(L.w);
  if ((threadIdx.x & 63u) == 0u) {
    atomicAdd(A.words + kContributing, (unsigned long long)__popcll(act));
    atomicAdd(A.words + kAdds, adds);
    if (beyond) atomicAdd(A.words + kBeyond, beyond);
    atomicAdd(A.words + kWeight, weight);
  }
}

// G lanes per vertex (a power of two, 1 .. 64), at most kPeakBlocks blocks that stride over the vertices: peak[v] = the largest
// cell of the row, window[v] = the smallest window that holds it (kNone: the row is empty); the cells above zero, the cells
// above free_count and the largest cell are kept in registers over the whole stride and leave as one atomic each per block
__global__ __launch_bounds__(kTimedBlock) void k_timed_peak(uint32_t V, uint32_t B, uint32_t G, uint32_t free_count, const uint32_t* __restrict__ cell,
                                                           uint32_t* __restrict__ peak, uint32_t* __restrict__ window, unsigned long long* __restrict__ words)
{
  __shared__ unsigned long long s_occ[kTimedBlock / 64], s_over[kTimedBlock / 64];
  __shared__ uint32_t s_big[kTimedBlock / 64];
  const size_t t = (size_t)blockIdx.x * kTimedBlock + threadIdx.x, groups = (size_t)gridDim.x * kTimedBlock / G;
  const uint32_t g = (uint32_t)(t % G), rounds = (uint32_t)((V + groups - 1) / groups);
  uint32_t big = 0u; unsigned long long occ = 0ull, over = 0ull;
  for (uint32_t r = 0; r < rounds; ++r) {                             // (the same count in every lane: the shuffles below meet whole groups)
    const size_t v = t / G + (size_t)r * groups;
    uint32_t m = 0u, at = mnav::kNone;
    if (v < V) {
      const uint32_t* row = cell + v * B;
      for (uint32_t k = g; k < B; k += G) {                           // ascending: the first window that attains the lane's maximum
        const uint32_t x = row[k];
        if (x > m) { m = x; at = k; }
        occ += x > 0u; over += x > free_count;
      }
    }
    for (uint32_t o = G >> 1; o > 0u; o >>= 1) {                      // (the group lies inside one wave: 64 % G == 0)
      const uint32_t m2 = __shfl_xor(m, o), at2 = __shfl_xor(at, o);
      if (m2 > m || (m2 == m && at2 < at)) { m = m2; at = at2; }
    }
    if (v < V && g == 0u) { peak[v] = m; window[v] = m ? at : mnav::kNone; }
    big = m > big ? m : big;
  }
  // the block's three figures: per wave, then one lane for the block -- a few thousand atomics on three addresses, not one per wave of cells
  occ = mnav_traffic::wave_sum64(occ); over = mnav_traffic::wave_sum64(over);
  for (int o = 32; o > 0; o >>= 1) { const uint32_t y = __shfl_xor(big, o); big = y > big ? y : big; }
  if ((threadIdx.x & 63u) == 0u) { s_occ[threadIdx.x >> 6] = occ; s_over[threadIdx.x >> 6] = over; s_big[threadIdx.x >> 6] = big; }
  __syncthreads();
  if (threadIdx.x == 0u) {
    for (int w = 1; w < kTimedBlock / 64; ++w) { occ += s_occ[w]; over += s_over[w]; big = s_big[w] > big ? s_big[w] : big; }
    if (occ) {
      atomicAdd(words + kOccupied, occ);
      if (over) atomicAdd(words + kOver, over);
      atomicMax(words + kLargest, (unsigned long long)big);
    }
  }
}

// after every add of the call: where each robot meets a cell above free_count, and where it is not the cell's holder
__global__ __launch_bounds__(kTimedBlock) void k_timed_report(Walk A)
{
  const uint32_t i = blockIdx.x * kTimedBlock + threadIdx.x, last = A.V - 1u;
  const Lane L = timed_lane(A, i);
  uint32_t u = L.u, over = 0u, yl = 0u, fv = mnav::kNone, fw = mnav::kNone; float ft = mnav::inf_f();
  for (uint32_t q = 0; q < L.visits; ++q) {
    const float d = L.dist[u];
    const uint32_t p = L.pred[u];
    const float t = timed_time(L.P, d, L.depart, L.pace);
    uint32_t k;
    if (timed_slot(t, A.tau, A.B, &k)) {
      const size_t c = (size_t)u * A.B + k;
      if (A.cell[c] > A.free_count) {
        ++over;
        if (A.holder[c] != L.key) { if (!yl) { fv = u; fw = k; ft = t; } ++yl; }
      }
    }
    u = p < last ? p : last;
  }
  if (i < A.n) { A.conflict[i] = over; A.yield[i] = yl; A.fy_vertex[i] = fv; A.fy_window[i] = fw; A.fy_time[i] = ft; }
  const unsigned long long ys = __ballot(yl != 0u);
  if ((threadIdx.x & 63u) == 0u && ys) atomicAdd(A.words + kYielding, (unsigned long long)__popcll(ys));
}

// the cells, the holders and the statistics of the last mnav_fleet_timed_traffic; dropped by mnav_upload_mesh
struct State {
  mnav::DevBuf<uint32_t> cell, holder; uint32_t B = 0; float tau = 0.f;            // V x B each; B == 0: no cells yet
  mnav::DevBuf<uint32_t> peak, window; mnav::DevBuf<unsigned long long> words;     // V each; the counters
  mnav::DevBuf<uint32_t> weight, key, conflict, yield, fy_vertex, fy_window; mnav::DevBuf<float> depart, pace, fy_time; size_t cap = 0;   // per robot
  unsigned long long T = 0ull;
  uint64_t contributing = 0, adds = 0, beyond = 0, occupied = 0, over = 0; uint32_t largest = 0, yielding = 0, windows = 0, built_index = 0;
  float ms_kernels = 0.f, ms_total = 0.f;
};

#endif  // __HIPCC__

}  // namespace mnav_timed
