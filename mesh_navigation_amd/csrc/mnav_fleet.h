// mnav_fleet.h -- fleet paths and fleet walks (mnav_fleet_paths, mnav_fleet_walks): many robots per resident field.
// A Dijkstra field is seeded at the goal, so below its cut it holds the vertex path of every robot inside it: robot i
// standing on vertex v of plan slots[i] gets pred[v], pred[pred[v]], ..., seed without another wave.  The per-robot rule
// (DESIGN.md section 3.12), first match wins; d / p = the plan's resident dist / pred, g = its seed, t = its target,
// cut = goal_cut(d[t], offset, t).cut:
//   1  v >= V                              INVALID_GOAL
//   2  the plan never reached the device   the plan's own code, length 0
//   3  v == g                              SUCCESS, length 0, potential 0
//   4  d[v] < cut, or v == t               p[v] == v: NO_PATH_FOUND; else SUCCESS, the chain to g, potential d[v]
//                                          (a chain that does not end within V hops: INTERNAL_ERROR)
//   5  d[v] == +inf and the wave ran out    NO_PATH_FOUND (ran out: cut == +inf, or no vertex holds a finite value at or above
//                                          the cut -- every vertex the wave reached was expanded, so v is not connected to g)
//   6  otherwise                           BEYOND_FIELD, length 0 (the tentative ring at or above the cut, and what the wave
//                                          never reached before it stopped)
// fleet_classify and fleet_write are the device's own source and the host mirror's (tests/test_fleet_model.py).
//
// Rule 5 with a finite cut needs a look at the whole field, so it is taken lazily: k_fleet_len marks such robots (and their
// plans) and calls them BEYOND_FIELD; only if there are any, k_fleet_open looks for a finite value at or above the cut in
// the marked plans and k_fleet_resolve turns the marked robots of the plans without one into NO_PATH_FOUND.
//
// Device shape: k_fleet_cut (one lane per plan: the cut from d[t]), k_fleet_len (one lane per robot: classify and count the
// hops; outcome counters by wave ballot, block sums of the lengths), k_fleet_scan + k_fleet_offsets (a deterministic 64-bit
// exclusive scan in robot order: one workgroup over the block sums, then every block over its own lengths), k_fleet_write
// (one lane per robot walks again and stores hop q at offset + len - 1 - q: list order, exact size, no reversal pass).  The
// chase is a dependent chain of 4-byte gathers; the plan's record comes from a small table and d / p are read through
// global pointers (GPtr), so no flat load is issued.
// The walks reuse k_backtrack as it is: k_fleet_jobs builds its job table from the slots on the device, k_fleet_walk_len
// turns its control words into statuses and lengths, the same scan gives the offsets and k_fleet_pack (one wave per robot)
// turns the scratch rows of walk_cap entries into the packed, seed-first output.
#pragma once
#include <cmath>
#include <cstdint>

#include "mnav_eval.h"

namespace mnav_fleet {

using mnav::GPtr;
using mnav::kNone;

constexpr uint32_t kSuccess = 0u, kInvalidStart = 52u, kInvalidGoal = 53u, kNoPath = 54u, kInternal = 60u, kBeyond = 70u;   // MNAV_*, include/mnav.h
constexpr int kFleetBlock = 256;   // robots per block of the length pass and of the scan
constexpr int kCounters = 4;       // served, beyond field, no path, invalid; word kCounters: robots marked for rule 5 with a finite cut
constexpr int kOpenBlocks = 32;    // blocks per marked plan of k_fleet_open
constexpr int kNoFace = -3;        // walk status: no face at the start

// One plan as the robots see it.  dist == null: the plan never reached the device and `code` is its own code.
struct Field { GPtr<const float> dist; GPtr<const uint32_t> pred; uint32_t seed, target; float cut; uint32_t code; };
struct Robot { uint32_t code, len; float potential; bool unreached; };   // unreached: d[v] == +inf under a finite cut (rule 5 or 6: fleet_open_value decides)

MNAV_HD void fleet_cut(Field& Fd, double offset)
{
  if (Fd.dist) Fd.cut = mnav::goal_cut(Fd.dist[Fd.target], offset, Fd.target).cut;
}

MNAV_HD Robot fleet_classify(const Field& Fd, uint32_t V, uint32_t v)
{
  Robot R; R.code = kInvalidGoal; R.len = 0u; R.potential = mnav::inf_f(); R.unreached = false;
  if (v >= V) return R;                                               // rule 1
  if (!Fd.dist) { R.code = Fd.code; return R; }                       // rule 2
  if (v == Fd.seed) { R.code = kSuccess; R.potential = 0.f; return R; }   // rule 3
  const float d = Fd.dist[v];
  if (d < Fd.cut || v == Fd.target) {                                 // rule 4
    R.potential = d;
    uint32_t u = Fd.pred[v];
    if (u == v) { R.code = kNoPath; return R; }
    uint32_t len = 1u;
    while (u != Fd.seed) {
      const uint32_t w = u < V ? Fd.pred[u] : u;
      if (w == u || len >= V) { R.code = kInternal; R.potential = mnav::inf_f(); return R; }
      u = w; ++len;
    }
    R.code = kSuccess; R.len = len;
    return R;
  }
  R.code = (!(d < mnav::inf_f()) && !(Fd.cut < mnav::inf_f())) ? kNoPath : kBeyond;   // rules 5 and 6
  R.unreached = !(d < mnav::inf_f()) && Fd.cut < mnav::inf_f();
  return R;
}
// a value that keeps a plan's wave from having run out: reached, but at or above the cut (such a vertex may not have been expanded)
MNAV_HD bool fleet_open_value(float d, float cut) { return d < mnav::inf_f() && d >= cut; }

// the `len` hops of a served robot in list order (seed first ... pred[v]); fleet_classify has walked the chain before
MNAV_HD void fleet_write(const Field& Fd, uint32_t v, uint32_t len, uint32_t* out)
{
  uint32_t u = v;
  for (uint32_t q = 0; q < len; ++q) { u = Fd.pred[u]; out[len - 1u - q] = u; }
}

// counter of a path code / of a walk status
MNAV_HD int fleet_outcome(uint32_t code) { return code == kSuccess ? 0 : code == kBeyond ? 1 : code == kNoPath ? 2 : 3; }
MNAV_HD int fleet_walk_outcome(int32_t status) { return status == 1 ? 0 : status == kNoFace ? 3 : 2; }

#if !defined(__HIP_DEVICE_COMPILE__)
// The host mirror of the scan, block by block as the device runs it: off[i] = the exclusive prefix sum of len in robot
// order, off[n] = the total.
inline void fleet_scan_host(uint32_t n, const uint32_t* len, unsigned long long* off)
{
  const uint32_t nb = (n + kFleetBlock - 1) / kFleetBlock;
  unsigned long long carry = 0;
  for (uint32_t b = 0; b < nb; ++b) {
    const uint32_t lo = b * kFleetBlock, hi = lo + kFleetBlock < n ? lo + kFleetBlock : n;
    unsigned long long in_block = 0;
    for (uint32_t i = lo; i < hi; ++i) { off[i] = carry + in_block; in_block += len[i]; }
    carry += in_block;
  }
  off[n] = carry;
}
// mnav_fleet_paths on host arrays: `fields` with host pointers and their cuts set; ids: null, or off[n] words
inline void fleet_paths_host(uint32_t n, uint32_t V, const Field* fields, const uint32_t* slot, const uint32_t* vtx, uint32_t* code, uint32_t* len,
                             float* potential, unsigned long long* off, uint32_t* ids, uint32_t* counters)
{
  for (uint32_t i = 0; i < n; ++i) {
    const Field& Fd = fields[slot[i]];
    Robot R = fleet_classify(Fd, V, vtx[i]);
    if (R.unreached) {                                                // rule 5 under a finite cut: did the wave run out?
      bool open = false;
      for (uint32_t u = 0; u < V && !open; ++u) open = fleet_open_value(Fd.dist[u], Fd.cut);
      if (!open) R.code = kNoPath;
    }
    code[i] = R.code; len[i] = R.len; potential[i] = R.potential;
    if (counters) counters[fleet_outcome(R.code)] += 1u;
  }
  fleet_scan_host(n, len, off);
  if (ids) for (uint32_t i = 0; i < n; ++i) if (len[i]) fleet_write(fields[slot[i]], vtx[i], len[i], ids + off[i]);
}
#endif

#if defined(__HIPCC__)

struct Paths {
  uint32_t n, V;
  const uint32_t* slot; const uint32_t* vtx; const Field* fields;
  uint32_t* code; uint32_t* len; float* potential; unsigned long long* bsum; uint32_t* cnt;
  int32_t* mark; uint32_t* need;   // per robot / per plan: waits for k_fleet_open's answer (rule 5 under a finite cut)
};
// One plan of a walk call: its resident vector map (null: the plan never reached the device) and the seed end.
struct WalkSlot { const float* vecmap; float seed[3]; uint32_t seed_face; };

// outcome counters of a block's robots: one ballot per counter, lane 0 of every wave adds (oc < 0: no robot in this lane)
__device__ __forceinline__ void fleet_count(int oc, uint32_t* cnt)
{
  for (int k = 0; k < kCounters; ++k) {
    const unsigned long long m = __ballot(oc == k);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(cnt + k, (uint32_t)__popcll(m));
  }
}
// the sum of one value per thread over the block, to bsum[blockIdx.x]
__device__ __forceinline__ void fleet_block_sum(uint32_t x, unsigned long long* bsum)
{
  __shared__ unsigned long long s[kFleetBlock];
  s[threadIdx.x] = x;
  __syncthreads();
  for (int o = kFleetBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) bsum[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(kFleetBlock) void k_fleet_cut(uint32_t m, Field* __restrict__ fields, double offset)
{
  const uint32_t s = blockIdx.x * kFleetBlock + threadIdx.x;
  if (s >= m) return;
  Field Fd = fields[s];
  fleet_cut(Fd, offset);
  fields[s].cut = Fd.cut;
}

__global__ __launch_bounds__(kFleetBlock) void k_fleet_len(Paths P)
{
  const uint32_t i = blockIdx.x * kFleetBlock + threadIdx.x;
  Robot R; R.code = kInvalidGoal; R.len = 0u; R.potential = 0.f; R.unreached = false;
  if (i < P.n) {
    const uint32_t s = P.slot[i];
    R = fleet_classify(P.fields[s], P.V, P.vtx[i]);
    P.code[i] = R.code; P.len[i] = R.len; P.potential[i] = R.potential; P.mark[i] = R.unreached ? 1 : 0;
    if (R.unreached) P.need[s] = 1u;
  }
  fleet_count(i < P.n ? fleet_outcome(R.code) : -1, P.cnt);
  const unsigned long long marked = __ballot(R.unreached);
  if ((threadIdx.x & 63u) == 0u && marked) atomicAdd(P.cnt + kCounters, (uint32_t)__popcll(marked));
  fleet_block_sum(R.len, P.bsum);
}

// kOpenBlocks blocks per plan, marked plans only: open[s] = 1 when the plan holds a finite value at or above its cut
__global__ __launch_bounds__(kFleetBlock) void k_fleet_open(uint32_t m, uint32_t V, const Field* __restrict__ fields, const uint32_t* __restrict__ need,
                                                           uint32_t* __restrict__ open)
{
  const uint32_t s = blockIdx.x / kOpenBlocks, b = blockIdx.x % kOpenBlocks;
  if (s >= m || !need[s]) return;
  const Field Fd = fields[s];
  bool any = false;
  for (uint32_t v = b * kFleetBlock + threadIdx.x; v < V; v += kOpenBlocks * kFleetBlock) any = any || fleet_open_value(Fd.dist[v], Fd.cut);
  const unsigned long long hit = __ballot(any);
  if ((threadIdx.x & 63u) == 0u && hit) atomicOr(open + s, 1u);
}

// the marked robots of the plans whose wave ran out: NO_PATH_FOUND (rule 5); lengths do not change
__global__ __launch_bounds__(kFleetBlock) void k_fleet_resolve(Paths P, const uint32_t* __restrict__ open)
{
  const uint32_t i = blockIdx.x * kFleetBlock + threadIdx.x;
  bool moved = false;
  if (i < P.n && P.mark[i] && !open[P.slot[i]]) { P.code[i] = kNoPath; moved = true; }
  const unsigned long long mv = __ballot(moved);
  if ((threadIdx.x & 63u) == 0u && mv) { atomicSub(P.cnt + 1, (uint32_t)__popcll(mv)); atomicAdd(P.cnt + 2, (uint32_t)__popcll(mv)); }
}

// One workgroup: bsum[0 .. nb) becomes its own exclusive scan on top of *base_in (null: 0); *total_out = the end value.
__global__ __launch_bounds__(kFleetBlock) void k_fleet_scan(uint32_t nb, unsigned long long* __restrict__ bsum, const unsigned long long* base_in,
                                                           unsigned long long* total_out)
{
  __shared__ unsigned long long s[kFleetBlock];
  __shared__ unsigned long long carry;
  const uint32_t t = threadIdx.x;
  if (t == 0) carry = base_in ? *base_in : 0ull;
  __syncthreads();
  for (uint32_t c = 0; c < nb; c += kFleetBlock) {
    const unsigned long long x = c + t < nb ? bsum[c + t] : 0ull;
    s[t] = x;
    __syncthreads();
    for (uint32_t o = 1; o < (uint32_t)kFleetBlock; o <<= 1) {
      const unsigned long long y = t >= o ? s[t - o] : 0ull;
      __syncthreads();
      s[t] += y;
      __syncthreads();
    }
    if (c + t < nb) bsum[c + t] = carry + s[t] - x;
    __syncthreads();
    if (t == kFleetBlock - 1) carry += s[t];
    __syncthreads();
  }
  if (t == 0) *total_out = carry;
}

// off[i] = bbase[block] + the exclusive scan of len inside the block
__global__ __launch_bounds__(kFleetBlock) void k_fleet_offsets(uint32_t n, const uint32_t* __restrict__ len, const unsigned long long* __restrict__ bbase,
                                                              unsigned long long* __restrict__ off)
{
  __shared__ unsigned long long s[kFleetBlock];
  const uint32_t t = threadIdx.x, i = blockIdx.x * kFleetBlock + t;
  const unsigned long long x = i < n ? len[i] : 0u;
  s[t] = x;
  __syncthreads();
  for (uint32_t o = 1; o < (uint32_t)kFleetBlock; o <<= 1) {
    const unsigned long long y = t >= o ? s[t - o] : 0ull;
    __syncthreads();
    s[t] += y;
    __syncthreads();
  }
  if (i < n) off[i] = bbase[blockIdx.x] + s[t] - x;
}

// ids holds off[n] words: robot i owns [off[i], off[i] + len[i])
__global__ __launch_bounds__(kFleetBlock) void k_fleet_write(Paths P, const unsigned long long* __restrict__ off, uint32_t* __restrict__ ids)
{
  const uint32_t i = blockIdx.x * kFleetBlock + threadIdx.x;
  if (i >= P.n) return;
  const uint32_t len = P.len[i];
  if (len) fleet_write(P.fields[P.slot[i]], P.vtx[i], len, ids + off[i]);
}

// jobs[j] for robot first + j: from its start to the seed end of its plan; no face at the start, or no plan: no job
__global__ __launch_bounds__(kFleetBlock) void k_fleet_jobs(uint32_t n, uint32_t F, const uint32_t* __restrict__ slot, const WalkSlot* __restrict__ ws,
                                                           const float* __restrict__ start_pos, const uint32_t* __restrict__ start_face, ::WalkJob* __restrict__ jobs)
{
  const uint32_t j = blockIdx.x * kFleetBlock + threadIdx.x;
  if (j >= n) return;
  const WalkSlot W = ws[slot[j]];
  const uint32_t f = start_face[j];
  ::WalkJob J;
  J.vecmap = f < F ? W.vecmap : nullptr;
  J.seed_face = W.seed_face; J.target_face = f;
  for (int k = 0; k < 3; ++k) { J.seed[k] = W.seed[k]; J.target[k] = start_pos[3 * (size_t)j + k]; }
  jobs[j] = J;
}

__global__ __launch_bounds__(kFleetBlock) void k_fleet_walk_len(uint32_t n, uint32_t F, const uint32_t* __restrict__ start_face, const int32_t* __restrict__ ctl,
                                                               int32_t* __restrict__ status, uint32_t* __restrict__ len, unsigned long long* __restrict__ bsum,
                                                               uint32_t* __restrict__ cnt)
{
  const uint32_t j = blockIdx.x * kFleetBlock + threadIdx.x;
  int32_t st = 0; uint32_t m = 0u;
  if (j < n) {
    st = ctl[2 * (size_t)j]; m = (uint32_t)ctl[2 * (size_t)j + 1];
    if (start_face[j] >= F) { st = kNoFace; m = 0u; }
    status[j] = st; len[j] = m;
  }
  fleet_count(j < n ? fleet_walk_outcome(st) : -1, cnt);
  fleet_block_sum(m, bsum);
}

// One wave per robot: its scratch row (walk order, start first) reversed into [off, off + len) of the packed output.  A
// row that would end beyond out_cap entries is left out (the call then reports the size it needs).
__global__ __launch_bounds__(64) void k_fleet_pack(uint32_t cap, const float* __restrict__ row_pos, const uint32_t* __restrict__ row_face,
                                                  const uint32_t* __restrict__ len, const unsigned long long* __restrict__ off, float* __restrict__ pos_out,
                                                  uint32_t* __restrict__ face_out, unsigned long long out_cap)
{
  const uint32_t j = blockIdx.x;
  const uint32_t m = len[j] < cap ? len[j] : cap;
  const unsigned long long o = off[j];
  if (o + m > out_cap) return;
  const float* rp = row_pos + 3 * (size_t)cap * j;
  const uint32_t* rf = row_face + (size_t)cap * j;
  for (uint32_t q = threadIdx.x; q < m; q += 64u) {
    const unsigned long long dst = o + (m - 1u - q);
    pos_out[3 * dst] = rp[3 * (size_t)q]; pos_out[3 * dst + 1] = rp[3 * (size_t)q + 1]; pos_out[3 * dst + 2] = rp[3 * (size_t)q + 2];
    face_out[dst] = rf[q];
  }
}

// what mnav_fleet_stats tells of the last fleet call
struct Stats {
  uint32_t outcome[kCounters] = { 0, 0, 0, 0 }, built_index = 0, chunks = 0; uint64_t entries = 0; float ms_kernels = 0.f, ms_total = 0.f;
};

// buffers and statistics of the last fleet call
struct State {
  mnav::DevBuf<uint32_t> slot, vtx, code, len, cnt, face; mnav::DevBuf<float> potential, pos; mnav::DevBuf<int32_t> status;
  mnav::DevBuf<unsigned long long> bsum, off; size_t cap = 0;                       // per robot
  mnav::DevBuf<Field> fields; mnav::DevBuf<WalkSlot> wslots; mnav::DevBuf<uint32_t> need; size_t slots_cap = 0;  // per plan
  mnav::DevBuf<uint32_t> ids; size_t ids_cap = 0;                                   // packed paths
  mnav::DevBuf<::WalkJob> jobs; mnav::DevBuf<int32_t> ctl; mnav::DevBuf<float> row_pos; mnav::DevBuf<uint32_t> row_face; size_t rows = 0, row_entries = 0;   // one chunk of walks
  mnav::DevBuf<float> out_pos; mnav::DevBuf<uint32_t> out_face; size_t out_cap = 0;   // packed walks
  mnav::Event ev[2]; bool have_ev = false;
  Stats stats;
};

#endif  // __HIPCC__

}  // namespace mnav_fleet
