// mnav_changelist.h -- the diff + compaction pass that ends the obstacle, clearance and border layers:
// the new cost and lethal flag of every vertex come from a Rule, are diffed against the layer slot and written into
// it, and the ids that changed are compacted into one ascending list.  Three kernels: k_chg_count<Rule> (changes and
// lethals per block), k_chg_scan (one workgroup: block offsets and the two totals), k_chg_emit<Rule> (ids, then the
// slot).  The host side is layer_change_list in mnav.hip.
//
// A Rule is a trivially copyable struct passed by value to the kernels:
//   __device__ float operator()(size_t v, uint8_t* lethal) const   the new cost and lethal flag of vertex v
//   static constexpr bool kCostBits   false: v changed iff its lethal flag differs from the slot's;
//                                     true: iff the flag or the cost bits differ, and every vertex of a fresh slot
#pragma once

namespace mnav_chg {

constexpr int kChgBlock = 256;            // lanes per workgroup
constexpr int kChgPer = 4;                // vertices per lane
// counters of one layer call (device words): the ray-cast kernels count kKept .. kOverflow (rays cast, rays that hit,
// lethal rays, waves whose traversal stack overflowed), k_chg_scan sets the two totals; one download brings back all
enum { kKept = 0, kHits, kLethalRays, kOverflow, kChanged, kLethal, kCounters };

inline uint32_t blocks(uint32_t V) { return (uint32_t)(((size_t)V + kChgBlock * kChgPer - 1) / (kChgBlock * kChgPer)); }

// per-context scratch, allocated by the first layer call after a mesh upload that needs it
struct Scratch {
  DevBuf<uint32_t> ids;        // V: change list
  DevBuf<uint32_t> blk;        // 3 x blocks: changed per block, lethal per block, exclusive offsets
  DevBuf<uint32_t> cnt;        // kCounters words
};

// exclusive scan of one value per lane over a block of kChgBlock lanes; *total = the block's sum
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* lds, uint32_t* total)
{
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t s = v;
  for (int off = 1; off < 64; off <<= 1) { const uint32_t u = __shfl_up(s, off); if (lane >= (uint32_t)off) s += u; }
  if (lane == 63) lds[w] = s;
  __syncthreads();
  uint32_t base = 0, all = 0;
  for (uint32_t k = 0; k < kChgBlock / 64; ++k) { if (k < w) base += lds[k]; all += lds[k]; }
  __syncthreads();
  *total = all;
  return base + s - v;
}

// the new cost `x` and flag `f` of vertex v against the slot
template <class Rule>
__device__ __forceinline__ bool changed(uint32_t fresh, size_t v, float x, uint8_t f, const float* __restrict__ cost, const uint8_t* __restrict__ lethal)
{
  if constexpr (Rule::kCostBits) return fresh || f != lethal[v] || __float_as_uint(x) != __float_as_uint(cost[v]);
  else return f != lethal[v];
}

// per block of kChgBlock * kChgPer vertices: how many vertices change, how many are lethal
template <class Rule>
__global__ __launch_bounds__(kChgBlock) void k_chg_count(uint32_t V, Rule rule, uint32_t fresh, const float* __restrict__ cost,
                                                         const uint8_t* __restrict__ lethal, uint32_t* __restrict__ blk, uint32_t nblk)
{
  __shared__ uint32_t lds[kChgBlock / 64];
  const size_t v0 = ((size_t)blockIdx.x * kChgBlock + threadIdx.x) * kChgPer;
  uint32_t c = 0, l = 0;
  for (int k = 0; k < kChgPer; ++k)
    if (v0 + k < V) {
      uint8_t f;
      const float x = rule(v0 + k, &f);
      c += changed<Rule>(fresh, v0 + k, x, f, cost, lethal);
      l += f;
    }
  uint32_t tc, tl;
  (void)block_scan(c, lds, &tc);
  (void)block_scan(l, lds, &tl);
  if (threadIdx.x == 0) { blk[blockIdx.x] = tc; blk[nblk + blockIdx.x] = tl; }
}

// one workgroup: exclusive offsets of the per-block change counts, totals into cnt
__global__ __launch_bounds__(kChgBlock) void k_chg_scan(uint32_t nblk, uint32_t* __restrict__ blk, uint32_t* __restrict__ cnt)
{
  __shared__ uint32_t lds[kChgBlock / 64];
  uint32_t carry = 0, lethal = 0;
  for (uint32_t b0 = 0; b0 < nblk; b0 += kChgBlock) {
    const uint32_t b = b0 + threadIdx.x;
    const uint32_t c = b < nblk ? blk[b] : 0, l = b < nblk ? blk[nblk + b] : 0;
    uint32_t tc, tl;
    const uint32_t ex = block_scan(c, lds, &tc);
    (void)block_scan(l, lds, &tl);
    if (b < nblk) blk[2 * nblk + b] = carry + ex;
    carry += tc; lethal += tl;
  }
  if (threadIdx.x == 0) { cnt[kChanged] = carry; cnt[kLethal] = lethal; }
}

// the changed ids in ascending order (block offset + lane prefix), then the slot's flags and costs
template <class Rule>
__global__ __launch_bounds__(kChgBlock) void k_chg_emit(uint32_t V, Rule rule, uint32_t fresh, float* __restrict__ cost, uint8_t* __restrict__ lethal,
                                                        const uint32_t* __restrict__ blk, uint32_t nblk, uint32_t* __restrict__ ids)
{
  __shared__ uint32_t lds[kChgBlock / 64];
  const size_t v0 = ((size_t)blockIdx.x * kChgBlock + threadIdx.x) * kChgPer;
  float x[kChgPer];
  uint8_t f[kChgPer], ch[kChgPer];
  uint32_t c = 0;
  for (int k = 0; k < kChgPer; ++k) {
    x[k] = 0.f; f[k] = 0; ch[k] = 0;
    if (v0 + k < V) {
      x[k] = rule(v0 + k, &f[k]);
      ch[k] = changed<Rule>(fresh, v0 + k, x[k], f[k], cost, lethal);
      c += ch[k];
    }
  }
  uint32_t tot;
  uint32_t pos = blk[2 * nblk + blockIdx.x] + block_scan(c, lds, &tot);
  for (int k = 0; k < kChgPer; ++k) {
    if (v0 + k >= V) break;
    if (ch[k]) ids[pos++] = (uint32_t)(v0 + k);
    lethal[v0 + k] = f[k];
    cost[v0 + k] = x[k];
  }
}

}  // namespace mnav_chg
