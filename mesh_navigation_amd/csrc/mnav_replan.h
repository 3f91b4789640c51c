// mnav_replan.h -- replan on a resident Dijkstra potential: the rewind level of every plan from the change
// log (k_replan_level), the rewind itself with the tiles' wake-up words (k_replan_rewind), and the two small kernels around
// them.  The tile rounds and the finalize pass then continue from the kept part of the field, unchanged.  Included by mnav.hip
// inside its anonymous namespace, after mnav_tiles.h and mnav_eval.h; not a stand-alone header.
#pragma once

// per plan: owned vertices kept / rewound from a finite value, tiles woken
struct ReplanCnt { unsigned long long kept, rewound; uint32_t woken, pad; };

// One thread per plan: the level word starts at the old cut (goal_cut of the old robot vertex -- every value strictly below
// it is final), the counters at zero, the control records as k_tile_init leaves them, except that the first round's minimum
// is collected by k_replan_rewind.
__global__ __launch_bounds__(kBlock) void k_replan_begin(const TilePlan* __restrict__ plans, uint32_t n, const uint32_t* __restrict__ old_target,
                                                         double old_offset, uint32_t* __restrict__ level, float* __restrict__ cut_old,
                                                         ReplanCnt* __restrict__ cnt)
{
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  const TilePlan& P = plans[p];
  const uint32_t tg = min(old_target[p], P.V - 1u);
  const float cut = goal_cut(P.dist[tg], old_offset, tg).cut;
  level[p] = f2u(cut); cut_old[p] = cut;
  ReplanCnt z; z.kept = 0ull; z.rewound = 0ull; z.woken = 0u; z.pad = 0u;
  cnt[p] = z;
  TCtl c0; memset(&c0, 0, sizeof(c0));
  c0.it = -1; c0.done = 0; c0.thr = -inf_f(); c0.thr_prev = -inf_f();
  P.ctl[0] = c0; P.ctl[1] = c0;
  TCnt e; e.minpend = kInfBits; e.acts = 0; e.sweeps = 0; e.pad = 0;
  P.cnt[0] = e; P.cnt[1] = e; P.cnt[2] = e;
}

// Both endpoints of the edges whose weight mnav_update_edge_weights replaced, appended to the change log.
__global__ __launch_bounds__(kBlock) void k_replan_log_edges(uint32_t n, const uint32_t* __restrict__ edge_ids, const uint32_t* __restrict__ edge_vtx,
                                                             uint32_t* __restrict__ out)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t e = edge_ids[i];
  out[2 * i] = edge_vtx[2 * (size_t)e]; out[2 * i + 1] = edge_vtx[2 * (size_t)e + 1];
}

// Rewind level: the smallest old value over the closed one-ring of every logged vertex.  grid (chunks of the log, plans),
// one lane per logged vertex; one atomicMin on the float bits per wave (values are >= 0: bit order is value order).
__global__ __launch_bounds__(kBlock) void k_replan_level(const TilePlan* __restrict__ plans, const uint32_t* __restrict__ log, uint32_t len,
                                                         const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ nbr_u,
                                                         uint32_t* __restrict__ level)
{
  const TilePlan& P = plans[blockIdx.y];
  MNAV_GLOBAL const float* g_dist = as_global((const float*)P.dist);
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < len;
  const uint32_t v = min(log[live ? i : 0u], P.V - 1u);               // (clamped: every load below is unconditional)
  const uint32_t rb = row_ptr[v], re = row_ptr[v + 1];
  float d = g_dist[v];
  for (uint32_t e = rb; e < re; ++e) d = fminf(d, g_dist[nbr_u[e]]);
  uint32_t m = live ? f2u(d) : kInfBits;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0 && m != kInfBits) atomicMin(&level[blockIdx.y], m);
}

// The rule of the rewind, for k_replan_rewind and for the warm start of the tile-batch engine (k_tb_warm, mnav_tb_warm.h): a
// vertex keeps its value iff it is the plan's seed (at 0) or the value lies strictly below the plan's level L.
__device__ __forceinline__ bool replan_keeps(bool is_seed, float d, float L) { return is_seed || d < L; }

// The rewind: one workgroup per (tile, plan).  An owned vertex is kept iff its value lies strictly below the plan's level
// (the seed always, at 0); every other one goes back to dist = +inf, pred = itself.  The halo is only read: its owners
// rewind it, and whether a value is kept does not depend on who reads it first (kept values are never written).  The tile's
// wake-up word is the smallest kept value among its owned and halo vertices when it also holds a vertex that is not kept
// (that value may still have something to propagate), +inf otherwise; every tile with a kept value is marked for the
// finalize pass (tlast = the finite mark of k_tile_round), which re-derives predecessors and the values beyond the new cut.
__global__ __launch_bounds__(kTileBlock) void k_replan_rewind(const TilePlan* __restrict__ plans, const Plan* __restrict__ fplans,
                                                              const uint32_t* __restrict__ level, ReplanCnt* __restrict__ cnt)
{
  const uint32_t t = blockIdx.x, p = blockIdx.y;
  const TilePlan& P = plans[p];
  const int tid = threadIdx.x;
  MNAV_GLOBAL const uint32_t* g_verts = as_global(P.verts);
  MNAV_GLOBAL const uint32_t* g_halo_verts = as_global(P.halo_verts);
  MNAV_GLOBAL float* g_dist = as_global(P.dist);
  MNAV_GLOBAL uint32_t* g_pred = as_global(fplans[p].pred);
  const float L = u2f(level[p]);
  const uint32_t seed = P.seed;
  const uint32_t v0 = P.vptr[t], nv = P.vptr[t + 1] - v0;
  const uint32_t h0 = P.hptr[t], nh = P.hptr[t + 1] - h0;
  uint32_t kmin = kInfBits, nk = 0, nr = 0, open = 0;                 // smallest kept value; owned kept / rewound; a vertex that is not kept
  for (uint32_t i = tid; i < nv; i += kTileBlock) {
    const uint32_t g = g_verts[v0 + i];
    const float d = g_dist[g];
    const bool is_seed = g == seed;
    if (replan_keeps(is_seed, d, L)) {
      if (is_seed && d != 0.0f) g_dist[g] = 0.0f;                     // dijkstra :276
      kmin = min(kmin, is_seed ? 0u : f2u(d)); ++nk;
    } else {
      if (d < inf_f()) { g_dist[g] = inf_f(); ++nr; }
      open = 1u;
    }
    g_pred[g] = g;                                                    // predecessors are re-derived by the finalize pass (kept tiles are all marked)
  }
  for (uint32_t i = tid; i < nh; i += kTileBlock) {
    const uint32_t g = g_halo_verts[h0 + i];
    const float d = g_dist[g];
    const bool is_seed = g == seed;
    if (replan_keeps(is_seed, d, L)) kmin = min(kmin, is_seed ? 0u : f2u(d));
    else open = 1u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, o));
    open |= (uint32_t)__shfl_xor((int)open, o);
    nk += (uint32_t)__shfl_xor((int)nk, o);
    nr += (uint32_t)__shfl_xor((int)nr, o);
  }
  __shared__ uint32_t s_kmin, s_open, s_nk, s_nr;
  if (tid == 0) { s_kmin = kInfBits; s_open = 0u; s_nk = 0u; s_nr = 0u; }
  __syncthreads();
  if ((tid & 63) == 0) { atomicMin(&s_kmin, kmin); atomicOr(&s_open, open); atomicAdd(&s_nk, nk); atomicAdd(&s_nr, nr); }
  __syncthreads();
  if (tid == 0) {
    const uint32_t km = s_kmin;
    const uint32_t wake = (s_open && km != kInfBits) ? km : kInfBits;
    P.pend[0][t] = wake;
    if (P.pend[1] != P.pend[0]) P.pend[1][t] = kInfBits;
    P.tlast[t] = (km != kInfBits) ? -3.0e38f : -inf_f();
    TCnt* const first = P.cnt + 2;                                    // what round 0 reads as the previous round's counters
    if (wake != kInfBits) { atomicMin(&first->minpend, wake); atomicAdd(&cnt[p].woken, 1u); }
    if (s_nk) atomicAdd(&cnt[p].kept, (unsigned long long)s_nk);
    if (s_nr) atomicAdd(&cnt[p].rewound, (unsigned long long)s_nr);
  }
}
