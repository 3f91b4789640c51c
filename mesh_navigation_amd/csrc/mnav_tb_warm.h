// mnav_tb_warm.h -- warm start of the tile-batch engine (mnav_tb.h) from rewound resident fields.
// A fresh batch starts from slices full of +inf, one 0 per plan with its ghost copies and one pending word per plan
// (k_tb_fill, k_tb_seed).  A rewound field is the same thing with more finite values and more pending tiles: k_tb_warm writes
// that state -- every word of every slice and every pending word of the sub-batch -- from the plans' resident V-sized
// potentials and their rewind levels, and the schedule kernels, the solve kernels, k_tb_finalize and the tail run unchanged.
// Included by mnav.hip after mnav_tb.h and mnav_replan.h (replan_keeps, ReplanCnt); not a stand-alone header.
#pragma once

constexpr int kWarmBlock = 256;           // four waves: one tile, 64 plans
constexpr uint32_t kWarmRun = 16;         // plans a wave walks with the tile's vertex ids in registers
constexpr uint32_t kWarmGroup = 2;        // plans whose loads are in flight together: 2 x up to 4 chunks per wave, 7 waves per SIMD (4 plans: 71 scalar registers spilled)
constexpr uint32_t kWarmChunks = 4;       // 64-slot chunks of a slice whose ids stay in registers (slices of up to 256 words; longer ones reload)

// What the pass reads besides the engine's own arguments, per plan of the sub-batch: the rewind level (float bits), the
// resident potential of the slot the plan stands in, and the counters it adds to (zeroed by the host).
struct TbWarm {
  const uint32_t* level; const float* const* dist; ReplanCnt* cnt;
  const uint32_t* verts; const uint32_t* ghost_gid; const uint32_t* order;   // tile order -> vertex id; the tiles' ghosts; the tiles by their smallest vertex id
  uint32_t T;
};

namespace tbw {

__device__ __forceinline__ uint32_t wave_min(uint32_t x)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = min(x, (uint32_t)__shfl_xor((int)x, o));
  return x;
}

// vertex id behind slot i of the tile's slice (kNone: padding)
__device__ __forceinline__ uint32_t slot_vertex(const TbTile& Tl, const TbWarm& W, uint32_t i)
{
  uint32_t v = kNone;
  if (i < Tl.nv) v = as_global(W.verts)[Tl.v0 + i];
  else if (i >= W.T && i - W.T < Tl.nh) v = as_global(W.ghost_gid)[Tl.goff + (i - W.T)];
  return v;
}

// The plans [p0, p1) of tile t, NCH chunks of 64 slots at a time.  Per group of kWarmGroup plans: NCH x kWarmGroup gathered
// loads at clamped indices, all issued before the first compare; then the rule, the contiguous stores, and the tile's word.
template <int NCH>
__device__ __forceinline__ void run(const tb::Args& A, const TbWarm& W, const TbTile& Tl, uint32_t t, uint32_t p0, uint32_t p1, uint32_t lane)
{
  const uint32_t nch = (Tl.sl + 63u) / 64u;
  const bool reload = nch > (uint32_t)NCH;                             // (a slice beyond NCH chunks: the ids are read again for every group)
  MNAV_GLOBAL const uint32_t* const g_level = as_global(W.level);
  MNAV_GLOBAL const uint32_t* const g_seed = as_global(A.seed);
  MNAV_GLOBAL uint32_t* const g_D = as_global((uint32_t*)A.D);
  uint32_t gid[NCH];
#pragma unroll
  for (int k = 0; k < NCH; ++k) gid[k] = slot_vertex(Tl, W, 64u * k + lane);
  uint32_t my_wake = kInfBits, my_kept = 0u, my_rew = 0u;              // lane q: the words of plan p0 + q
  for (uint32_t g = p0; g < p1; g += kWarmGroup) {
    float L[kWarmGroup]; uint32_t sd[kWarmGroup], km[kWarmGroup], nk[kWarmGroup], nr[kWarmGroup];
    uint32_t open[kWarmGroup];
    MNAV_GLOBAL const float* dp[kWarmGroup];
#pragma unroll
    for (uint32_t q = 0; q < kWarmGroup; ++q) {
      const uint32_t p = min(g + q, p1 - 1u);                          // (clamped: a short last group repeats its last plan, and stores nothing for it)
      L[q] = u2f(g_level[p]); sd[q] = g_seed[p]; dp[q] = as_global(W.dist[p]);
      km[q] = kInfBits; nk[q] = 0u; nr[q] = 0u; open[q] = 0u;
    }
    for (uint32_t c0 = 0; c0 < nch; c0 += (uint32_t)NCH) {
      if (reload) {
#pragma unroll
        for (int k = 0; k < NCH; ++k) gid[k] = slot_vertex(Tl, W, 64u * (c0 + k) + lane);
      }
      float d[kWarmGroup][NCH];
#pragma unroll
      for (uint32_t q = 0; q < kWarmGroup; ++q)
#pragma unroll
        for (int k = 0; k < NCH; ++k) d[q][k] = dp[q][gid[k] != kNone ? gid[k] : 0u];
#pragma unroll
      for (uint32_t q = 0; q < kWarmGroup; ++q) {
        const bool live = g + q < p1;
        const size_t base = (size_t)Tl.soff * A.NP + (size_t)min(g + q, p1 - 1u) * Tl.sl;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
          const uint32_t i = 64u * (c0 + k) + lane;
          const bool valid = gid[k] != kNone, is_seed = valid && gid[k] == sd[q];
          const bool keep = valid && replan_keeps(is_seed, d[q][k], L[q]);
          const uint32_t bits = keep ? (is_seed ? 0u : f2u(d[q][k])) : kInfBits;   // (the seed always at 0: dijkstra :276)
          if (live && i < Tl.sl) g_D[base + i] = bits;
          km[q] = min(km[q], bits);
          const bool own = i < Tl.nv;
          nk[q] += (uint32_t)__popcll(__ballot(own && keep));
          nr[q] += (uint32_t)__popcll(__ballot(own && !keep && d[q][k] < inf_f()));
          open[q] |= __any(own && !keep) ? 1u : 0u;
        }
      }
    }
#pragma unroll
    for (uint32_t q = 0; q < kWarmGroup; ++q) {
      const uint32_t m = wave_min(km[q]);
      const uint32_t wake = (open[q] && m != kInfBits) ? m : kInfBits;   // a kept value next to a vertex that is not kept may still have something to propagate
      if (lane == g - p0 + q) { my_wake = wake; my_kept = nk[q]; my_rew = nr[q]; }
    }
  }
  if (lane < p1 - p0) {
    const uint32_t p = p0 + lane;
    A.pend[(size_t)t * A.NP + p] = my_wake;
    if (my_wake != kInfBits) {
      A.pflag[(size_t)t * A.nblk + (p >> 6)] = 1;
      atomicMin(&A.marr[0][p], my_wake);
      A.ctl->n_cand[0] = 1u;                                           // (a flag: see k_tb_sched)
      atomicAdd(&W.cnt[p].woken, 1u);
    }
    if (my_kept) atomicAdd(&W.cnt[p].kept, (unsigned long long)my_kept);
    if (my_rew) atomicAdd(&W.cnt[p].rewound, (unsigned long long)my_rew);
  }
}

}  // namespace tbw

// The warm state of a sub-batch, instead of k_tb_fill(D), k_tb_fill(pend) and k_tb_seed: for every (tile t, plan p) EVERY word of
// the slice D[soff * NP + p * sl .. + sl) and of pend[t * NP + p].  Slot i < nv holds the rule of k_replan_rewind (replan_keeps:
// the seed at 0, a value strictly below the plan's level, +inf otherwise) applied to dist_p[verts[v0 + i]], slot T <= i < T + nh
// the same for the ghost ghost_gid[goff + i - T], every other slot +inf.  Values at or above the level are dropped, so the
// tentative values the finalize pass left beyond the old cut never enter.  The wake-up word is the smallest kept value among the
// tile's owned and ghost slots when the tile owns a vertex that is not kept, +inf otherwise: too low a value is safe (k_tb_sched
// drops only what lies above the goal bound), a missing one would be a wrong field.  Counters per plan as ReplanCnt defines them:
// owned vertices kept (seed included), owned vertices dropped from a finite value, (tile, plan) pairs woken.
//
// A pure HBM pass: per slice word and plan one gathered 4-byte read and one contiguous 4-byte write -- NP * S * 8 bytes, plus the
// id tables (4 bytes per slice word and 64 plans) and 4 bytes per (tile, plan) of pending words.  One workgroup per (tile, 64
// plans), a wave per run of 16 plans, lanes over the slice's slots with the vertex ids in registers; consecutive workgroups take
// the tiles in the order of their smallest vertex id (k_tb_finalize's order), so that the gathered reads of one plan's field by
// neighbouring tiles meet in the L2.  No LDS (the reductions are ballots and one cross-lane minimum per plan), no scratch.
__global__ __launch_bounds__(kWarmBlock) void k_tb_warm(tb::Args A, TbWarm W)
{
  const uint32_t lane = threadIdx.x & 63u, wave = tb::rfl(threadIdx.x >> 6);   // (uniform: the plans' words come through scalar loads)
  const uint32_t pblk = blockIdx.x / A.ntiles;
  const uint32_t t = min(as_global(W.order)[blockIdx.x - pblk * A.ntiles], A.ntiles - 1u);
  const uint32_t p0 = pblk * 64u + wave * kWarmRun;
  if (p0 >= A.NP) return;                                              // (uniform over the wave)
  const uint32_t p1 = min(p0 + kWarmRun, A.NP);
  const TbTile Tl = A.tiles[t];
  const uint32_t nch = (Tl.sl + 63u) / 64u;
  if (nch <= 2u) tbw::run<2>(A, W, Tl, t, p0, p1, lane);
  else if (nch == 3u) tbw::run<3>(A, W, Tl, t, p0, p1, lane);
  else tbw::run<(int)kWarmChunks>(A, W, Tl, t, p0, p1, lane);
}
