// mnav_graph.h -- the resident layer graph: LayerManager (layer_manager.cpp:153-263) + MeshMap::layerChanged
// (mesh_map.cpp:454-493) on the device.  Kernels and state; the host side is mnav_graph_capi.h.  Included by mnav.hip inside
// its anonymous namespace, after mnav_changelist.h (block_scan, the block geometry) and mnav_map_kernels.h (infl_fading).
//
// A node pass is the change-list pass of mnav_changelist.h with two differences: a Rule may decline a vertex (a vertex
// outside the incoming change list is neither read nor written), and the second counter is the number of vertices whose
// lethal flag flipped, which is what a dependent inflation node asks.  Three kernels: k_node_count<Rule>, k_node_scan,
// k_node_emit<Rule>.  A Rule is a trivially copyable struct passed by value:
//   __device__ bool operator()(size_t v, float* cost, uint8_t* lethal) const   false: v is not part of this pass
// With CombRule over a stamped id set these are the issue's "k_comb_slot_ids"; k_comb_slot is the full pass of
// mnav_map_compute.
#pragma once

namespace mnav_map {

using mnav_chg::kChgBlock;
using mnav_chg::kChgPer;
using mnav_chg::block_scan;
using mnav_chg::blocks;

constexpr uint32_t kMaxInputs = 8, kMaxLayers = 64;
// device counters of one node pass (kOut .. kActive: set by k_node_scan) and of one k_scatter_layer (kScatterFlipped)
enum { kOut = 0, kFlipped, kActive, kScatterFlipped, kCounters };

// the inputs of one combination node: resident from mnav_map_configure on
struct CombTab {
  const float* cost[kMaxInputs];
  const uint8_t* lethal[kMaxInputs];
  float w[kMaxInputs];
  uint32_t n;
  int mode;                                                          // 0 max, 1 weighted sum
};

// CombinationLayer over layer slots: the cost with k_combine_resident's arithmetic (from 0.0f, inputs in order, max or
// += w * x, no contraction), the lethal flag the OR of the inputs' (combination_layer.cpp:73-79, :122-139)
__device__ __forceinline__ float comb_eval(const CombTab& T, size_t v, uint8_t* lethal)
{
  float cost = 0.0f;                                                 // defaultValue(), combination_layer.h:52,94
  uint8_t f = 0;
  for (uint32_t l = 0; l < T.n; ++l) {
    const float tmp = T.cost[l][v];
    if (T.mode == 0) cost = (cost < tmp) ? tmp : cost;               // std::max(cost, tmp) :66
    else cost += T.w[l] * tmp;                                       // :206
    f |= T.lethal[l][v] != 0;
  }
  *lethal = f;
  return cost;
}

struct CombRule {
  const CombTab* __restrict__ tab;
  const uint8_t* __restrict__ stamp;                                 // the incoming change list as V flags
  __device__ __forceinline__ bool operator()(size_t v, float* cost, uint8_t* lethal) const
  {
    if (!stamp[v]) return false;
    *cost = comb_eval(*tab, v, lethal);
    return true;
  }
};

// InflationLayer::onInputChanged (inflation_layer.cpp:153-176) after the wave: riskiness = fading(distance), lethal flags =
// the input's.  Reads neither the slot's costs nor its flags, so it is safe on a fresh slot.
struct InflRule {
  const float* __restrict__ dist;
  const uint8_t* __restrict__ in_lethal;
  double inflation_radius, inscribed_radius, inscribed_value, lethal_value, cost_scaling_factor;
  __device__ __forceinline__ bool operator()(size_t v, float* cost, uint8_t* lethal) const
  {
    *cost = infl_fading(dist[v], inflation_radius, inscribed_radius, inscribed_value, lethal_value, cost_scaling_factor);
    *lethal = in_lethal[v];
    return true;
  }
};

// One vertex of a node pass: bit 0 = part of the pass, bit 1 = cost bits or flag differ from the slot, bit 2 = the flag
// flipped.  A fresh slot holds nothing: every vertex of the pass changed, against an empty lethal set.
template <class Rule>
__device__ __forceinline__ uint32_t node_vertex(const Rule& rule, uint32_t fresh, size_t v, const float* __restrict__ cost,
                                                const uint8_t* __restrict__ lethal, float* x, uint8_t* f)
{
  if (!rule(v, x, f)) return 0;
  const bool was = !fresh && lethal[v] != 0, is = *f != 0;
  const bool ch = fresh || was != is || __float_as_uint(*x) != __float_as_uint(cost[v]);
  return 1u | (ch ? 2u : 0u) | (was != is ? 4u : 0u);
}

// blk: 4 x nblk words -- changed, flipped and active vertices per block, exclusive offsets of the changed ones
template <class Rule>
__global__ __launch_bounds__(kChgBlock) void k_node_count(uint32_t V, Rule rule, uint32_t fresh, const float* __restrict__ cost,
                                                          const uint8_t* __restrict__ lethal, uint32_t* __restrict__ blk, uint32_t nblk)
{
  __shared__ uint32_t lds[kChgBlock / 64];
  const size_t v0 = ((size_t)blockIdx.x * kChgBlock + threadIdx.x) * kChgPer;
  uint32_t c = 0, fl = 0, a = 0;
  for (int k = 0; k < kChgPer; ++k)
    if (v0 + k < V) {
      float x; uint8_t f;
      const uint32_t r = node_vertex(rule, fresh, v0 + k, cost, lethal, &x, &f);
      a += r & 1u; c += (r >> 1) & 1u; fl += (r >> 2) & 1u;
    }
  uint32_t tc, tf, ta;
  (void)block_scan(c, lds, &tc);
  (void)block_scan(fl, lds, &tf);
  (void)block_scan(a, lds, &ta);
  if (threadIdx.x == 0) { blk[blockIdx.x] = tc; blk[nblk + blockIdx.x] = tf; blk[2 * nblk + blockIdx.x] = ta; }
}

// one workgroup: exclusive offsets of the per-block change counts, the three totals into cnt
__global__ __launch_bounds__(kChgBlock) void k_node_scan(uint32_t nblk, uint32_t* __restrict__ blk, uint32_t* __restrict__ cnt)
{
  __shared__ uint32_t lds[kChgBlock / 64];
  uint32_t carry = 0, flipped = 0, active = 0;
  for (uint32_t b0 = 0; b0 < nblk; b0 += kChgBlock) {
    const uint32_t b = b0 + threadIdx.x;
    const uint32_t c = b < nblk ? blk[b] : 0, f = b < nblk ? blk[nblk + b] : 0, a = b < nblk ? blk[2 * nblk + b] : 0;
    uint32_t tc, tf, ta;
    const uint32_t ex = block_scan(c, lds, &tc);
    (void)block_scan(f, lds, &tf);
    (void)block_scan(a, lds, &ta);
    if (b < nblk) blk[3 * nblk + b] = carry + ex;
    carry += tc; flipped += tf; active += ta;
  }
  if (threadIdx.x == 0) { cnt[kOut] = carry; cnt[kFlipped] = flipped; cnt[kActive] = active; }
}

// the changed ids in ascending order (block offset + lane prefix), then the slot's flags and costs of the pass's vertices
template <class Rule>
__global__ __launch_bounds__(kChgBlock) void k_node_emit(uint32_t V, Rule rule, uint32_t fresh, float* __restrict__ cost, uint8_t* __restrict__ lethal,
                                                         const uint32_t* __restrict__ blk, uint32_t nblk, uint32_t* __restrict__ ids)
{
  __shared__ uint32_t lds[kChgBlock / 64];
  const size_t v0 = ((size_t)blockIdx.x * kChgBlock + threadIdx.x) * kChgPer;
  float x[kChgPer];
  uint8_t f[kChgPer];
  uint32_t r[kChgPer], c = 0;
  for (int k = 0; k < kChgPer; ++k) {
    x[k] = 0.f; f[k] = 0; r[k] = 0;
    if (v0 + k < V) {
      r[k] = node_vertex(rule, fresh, v0 + k, cost, lethal, &x[k], &f[k]);
      c += (r[k] >> 1) & 1u;
    }
  }
  uint32_t tot;
  uint32_t pos = blk[3 * nblk + blockIdx.x] + block_scan(c, lds, &tot);
  for (int k = 0; k < kChgPer; ++k) {
    if (v0 + k >= V) break;
    if (r[k] & 2u) ids[pos++] = (uint32_t)(v0 + k);                 // pos < the total of k_node_scan <= V
    if (r[k] & 1u) { lethal[v0 + k] = f[k]; cost[v0 + k] = x[k]; }
  }
}

// the full pass of a combination node (mnav_map_compute)
__global__ __launch_bounds__(kBlock) void k_comb_slot(uint32_t V, const CombTab* __restrict__ tab, float* __restrict__ cost, uint8_t* __restrict__ lethal)
{
  const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= V) return;
  uint8_t f;
  cost[v] = comb_eval(*tab, v, &f);
  lethal[v] = f;
}

// The union of ascending id lists is a V-byte stamp: set by each list before the pass that reads it, cleared by the same
// lists after it (value 0), never by a V-sized memset.  Every id of a list is < V (k_node_emit / the host's check).
__global__ __launch_bounds__(kBlock) void k_stamp_ids(uint32_t n, const uint32_t* __restrict__ ids, uint8_t value, uint8_t* __restrict__ stamp)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) stamp[ids[i]] = value;
}

// mnav_map_update_layer: n distinct ids (< V, checked on the host) take their new costs and, with `flags`, lethal flags
__global__ __launch_bounds__(kBlock) void k_scatter_layer(uint32_t n, const uint32_t* __restrict__ ids, const float* __restrict__ values,
                                                          const uint8_t* __restrict__ flags, float* __restrict__ cost, uint8_t* __restrict__ lethal,
                                                          uint32_t* __restrict__ cnt)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t v = ids[i];
  cost[v] = values[i];
  if (flags) {
    const uint8_t f = flags[i] != 0;
    if ((lethal[v] != 0) != (f != 0)) atomicAdd(&cnt[kScatterFlipped], 1u);
    lethal[v] = f;
  }
}

__global__ __launch_bounds__(kBlock) void k_gather_costs(uint32_t n, const uint32_t* __restrict__ ids, const float* __restrict__ cost,
                                                         float* __restrict__ values)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) values[i] = cost[ids[i]];
}

// what a diffing pass leaves for the host: the device list, and (pinned) the counters of k_node_scan
struct Diff {
  uint32_t* ids; uint32_t* blk; uint32_t* cnt; uint32_t* h_cnt;
};

struct Node {
  uint32_t layer = 0, kind = 0, n_in = 0;
  uint32_t in[kMaxInputs] = {};
  float w[kMaxInputs] = {};
  double p[5] = {};                                                  // inflation_radius .. cost_scaling_factor
  int tab = -1;                                                      // combination: index into State::d_tabs
  DevBuf<uint32_t> ids;                                              // V: the outgoing change list of a derived node / an updated input
  // the running update call
  const uint32_t* out = nullptr; uint32_t n_out = 0, flipped = 0;
};

struct State {
  bool configured = false, computed = false, stale = false;
  std::vector<Node> order;                                           // inputs before users
  int pos[kMaxLayers];                                               // slot -> index into order, -1: not a node
  uint32_t default_layer = 0;
  double edge_cost_factor = 0.0;
  bool have_invalid = false; std::vector<uint8_t> h_invalid; DevBuf<uint8_t> d_invalid;
  DevBuf<CombTab> d_tabs;
  DevBuf<uint8_t> stamp;                                             // V, all zero between passes
  DevBuf<uint32_t> blk, cnt; PinnedBuf<uint32_t> h_cnt;              // 4 x blocks, kCounters, kCounters
  DevBuf<float> vals;                                                // V: the default layer's values on D
  DevBuf<float> up_vals; DevBuf<uint8_t> up_flags; size_t up_cap = 0;   // mnav_map_update_layer's staging
  std::vector<uint32_t> h_ids; std::vector<float> h_vals;            // D on the host
  Event ev[2];
  // the last update call
  uint32_t waves = 0, recombined = 0, default_changed = 0, edges_reweighted = 0; float ms_total = 0.f, ms_wave = 0.f;
};

}  // namespace mnav_map
