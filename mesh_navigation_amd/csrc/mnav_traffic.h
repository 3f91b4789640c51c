// mnav_traffic.h -- fleet traffic (mnav_fleet_traffic, mnav_layer_traffic, mnav_map_traffic): how many planned paths
// cross each vertex, and the congestion cost made of the excess.
// The context owns V uint32 counts c and the 64-bit total T of the accumulated weight.  Robot i of weight w_i contributes
// iff mnav_fleet_paths gives it MNAV_SUCCESS with a finite potential (rules 3 and 4 of mnav_fleet.h; never rule 2's
// seed == target plans, whose potential is +inf); it adds w_i to c[v_i] and to c[u] for every id u of its path
// pred[v], pred[pred[v]], ..., seed: len + 1 adds, one for a robot on the seed.  Integer sums do not depend on their
// order: the counts are the same bits whatever the schedule of the atomics.
// The cost rule (traffic_cost): e = c > free_count ? c - free_count : 0; 0.0f when e == 0, else
// fminf((float)e * gain, cap) -- one round-to-nearest conversion, one float multiply, no contraction.  Never lethal.
// traffic_contributes, traffic_cost and -- over fleet_classify -- traffic_counts_host are the device's own source and the
// host mirror's (tests/test_traffic_model.py).
//
// Device shape: classification and hop counts are k_fleet_cut / k_fleet_len (and k_fleet_open / _resolve for rule 5) of
// mnav_fleet.h.  k_traffic_add: one lane per robot walks its `len` hops -- the count is known, no walk is unbounded -- and
// issues one no-return atomicAdd per vertex; pred is read through GPtr (global loads), the per-robot words are loaded
// unconditionally at the clamped robot index.  No id array exists: the scratch is O(n).  The last add of every
// contributor lands on its plan's seed; with `combine` (option traffic_combine, off by default: it measured within 1 % either
// way) a wave whose contributors all ended on one vertex sums their weights by a wave reduction and issues one add.  k_traffic_stats: one pass over the counts for the occupied vertices and the
// peak, by wave ballot / wave maximum with one atomic per wave.  No kernel waits for another workgroup.
#pragma once
#include <cmath>
#include <cstdint>

#include "mnav_fleet.h"

namespace mnav_traffic {

using mnav_fleet::Field;
using mnav_fleet::Robot;

constexpr int kTrafficBlock = 256;                       // robots / vertices per block
constexpr unsigned long long kMaxTotal = 0xFFFFFFFFull;  // T never exceeds it: no count can wrap
enum { kContributing = 0, kAdds, kWeight, kSums };       // 64-bit sums of one call (device words)
enum { kOccupied = 0, kPeak, kVertexStats };             // 32-bit statistics of the counts

// does a robot with this outcome of mnav_fleet_paths add its weight?
MNAV_HD bool traffic_contributes(uint32_t code, float potential) { return code == mnav_fleet::kSuccess && potential < mnav::inf_f(); }

MNAV_HD float traffic_cost(uint32_t c, uint32_t free_count, float gain, float cap)
{
  if (c <= free_count) return 0.f;
  return fminf((float)(c - free_count) * gain, cap);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// mnav_fleet_traffic on host arrays: `fields` with host pointers and their cuts set, c (V words) and *T the context's
// state.  Returns -1 with nothing touched when the weights do not fit the counters; sums: kSums words (may be null).
inline int traffic_counts_host(uint32_t n, uint32_t V, const Field* fields, const uint32_t* slot, const uint32_t* vtx, const uint32_t* weights, int accumulate,
                               uint32_t* c, unsigned long long* T, uint32_t* code, float* potential, unsigned long long* sums)
{
  unsigned long long all = accumulate ? *T : 0ull;
  for (uint32_t i = 0; i < n; ++i) all += weights ? weights[i] : 1u;   // (n < 2^31 words of 32 bits: no 64-bit overflow)
  if (all > kMaxTotal) return -1;
  if (!accumulate) { for (uint32_t v = 0; v < V; ++v) c[v] = 0u; *T = 0ull; }
  unsigned long long s[kSums] = { 0ull, 0ull, 0ull };
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
    if (!traffic_contributes(R.code, R.potential) || !w) continue;
    uint32_t u = vtx[i];
    for (uint32_t q = 0; q < R.len; ++q) { c[u] += w; u = Fd.pred[u]; }
    c[u] += w;                                                        // the seed
    s[kContributing] += 1ull; s[kAdds] += (unsigned long long)R.len + 1ull; s[kWeight] += w;
  }
  *T += s[kWeight];
  if (sums) for (int k = 0; k < kSums; ++k) sums[k] = s[k];
  return 0;
}
#endif

#if defined(__HIPCC__)

struct Add {
  uint32_t n, V;
  const uint32_t* slot; const uint32_t* vtx; const Field* fields;
  const uint32_t* code; const uint32_t* len; const float* potential;   // of k_fleet_len (a later k_fleet_resolve moves no MNAV_SUCCESS)
  const uint32_t* weight;                                               // null: every robot weighs 1
  uint32_t* c; unsigned long long* sums;
  uint32_t combine;                                                     // one add per wave whose contributors end on one vertex
};

// the sum of one value per lane over the wave, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t x)
{
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long x)
{
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)x, o), hi = __shfl_xor((uint32_t)(x >> 32), o);
    x += ((unsigned long long)hi << 32) | lo;
  }
  return x;
}

__global__ __launch_bounds__(kTrafficBlock) void k_traffic_add(Add A)
{
  const uint32_t i = blockIdx.x * kTrafficBlock + threadIdx.x, lane = threadIdx.x & 63u;
  const uint32_t j = i < A.n ? i : A.n - 1u;                          // clamped (n >= 1): the loads below are unconditional
  const uint32_t s = A.slot[j], v = A.vtx[j], code = A.code[j], len = A.len[j];
  const float pot = A.potential[j];
  uint32_t w = A.weight ? A.weight[j] : 1u;                            // (a wave-uniform branch)
  if (i >= A.n || !traffic_contributes(code, pot)) w = 0u;
  const mnav::GPtr<const uint32_t> pred = A.fields[s].pred;
  const uint32_t hops = w ? len : 0u, last = A.V - 1u;
  uint32_t u = v < last ? v : last;                                   // a contributor stands on a vertex (rule 1)
  for (uint32_t q = 0; q < hops; ++q) {
    atomicAdd(A.c + u, w);
    const uint32_t p = pred[u];
    u = p < last ? p : last;                                          // (fleet_classify has walked this chain: every id is a vertex)
  }
  // u: the plan's seed for every contributor
  const unsigned long long act = __ballot(w != 0u);
  if (!act) return;
  bool single = false;
  if (A.combine) {
    const uint32_t u0 = __shfl(u, __ffsll((long long)act) - 1);
    single = __ballot(w == 0u || u == u0) == ~0ull;
    if (single) {
      const uint32_t sum = wave_sum(w);                               // (at most T <= 2^32 - 1)
      if (lane == (uint32_t)(__ffsll((long long)act) - 1)) atomicAdd(A.c + u0, sum);
    }
  }
  if (!single && w) atomicAdd(A.c + u, w);
  const unsigned long long adds = wave_sum64(w ? (unsigned long long)hops + 1ull : 0ull), weight = wave_sum64(w);
  if (lane == 0u) {
    atomicAdd(A.sums + kContributing, (unsigned long long)__popcll(act));
    atomicAdd(A.sums + kAdds, adds);
    atomicAdd(A.sums + kWeight, weight);
  }
}

// vertices with a count above zero and the largest count: one ballot and one maximum per wave
__global__ __launch_bounds__(kTrafficBlock) void k_traffic_stats(uint32_t V, const uint32_t* __restrict__ c, uint32_t* __restrict__ vstat)
{
  const uint32_t v = blockIdx.x * kTrafficBlock + threadIdx.x;
  const uint32_t x = c[v < V ? v : V - 1u];                           // (V >= 1; unconditional load at the clamped index)
  uint32_t m = v < V ? x : 0u;
  const unsigned long long occ = __ballot(m != 0u);
  if (!occ) return;
  for (int o = 32; o > 0; o >>= 1) { const uint32_t y = __shfl_xor(m, o); m = y > m ? y : m; }
  if ((threadIdx.x & 63u) == 0u) { atomicAdd(vstat + kOccupied, (uint32_t)__popcll(occ)); atomicMax(vstat + kPeak, m); }
}

// the change-list rule of mnav_layer_traffic (mnav_changelist.h)
struct TrafficRule {
  static constexpr bool kCostBits = true;
  const uint32_t* __restrict__ c;
  uint32_t free_count; float gain, cap;
  __device__ __forceinline__ float operator()(size_t v, uint8_t* lethal) const { *lethal = 0; return traffic_cost(c[v], free_count, gain, cap); }
};

// the counts and the statistics of the last mnav_fleet_traffic; dropped by mnav_upload_mesh
struct State {
  mnav::DevBuf<uint32_t> c, weight, vstat; mnav::DevBuf<unsigned long long> sums; size_t cap = 0;   // V counts; per robot; the two sets of counters
  unsigned long long T = 0ull;
  uint32_t contributing = 0, occupied = 0, peak = 0, built_index = 0; uint64_t adds = 0; float ms_kernels = 0.f, ms_total = 0.f;
};

#endif  // __HIPCC__

}  // namespace mnav_traffic
