// mnav_replan_each.h -- the per-plan replan: after the level pass of mnav_replan.h every plan of the batch is
// KEPT, REPAIRED or FRESH (k_replan_classify, with an ordered compaction into three lists of plan indices), and the records of
// the plans that go on are gathered into compacted arrays (k_replan_gather) over which the rewind, the tile rounds, the
// finalize pass and the tail kernels run unchanged.  Included by mnav.hip after mnav_replan.h; not a stand-alone header.
#pragma once

constexpr uint32_t kEachKept = 0u, kEachRepaired = 1u, kEachFresh = 2u;
constexpr int kClassifyBlock = 1024;

static_assert(sizeof(Plan) % 4 == 0 && sizeof(TilePlan) % 4 == 0 && offsetof(TilePlan, ctl) % 8 == 0 && sizeof(GPtr<TCtl>) == 8, "k_replan_gather copies the records word by word");

// The level word of a plan whose logged vertices all lie BEYOND its old cut: the float above the cut (the cut itself when that
// is +inf).  k_replan_level only ever lowers the word, so a word still at this value tells that no logged one-ring holds a value
// at or below the cut -- a value AT the cut may belong to an expanded source (expanded_source, mnav_eval.h).
__device__ __forceinline__ uint32_t replan_open_level(float cut) { return cut < inf_f() ? f2u(cut) + 1u : kInfBits; }

// One thread per plan, between k_replan_begin and k_replan_level: opens the level word above the cut.
__global__ __launch_bounds__(kBlock) void k_replan_open(uint32_t n, const float* __restrict__ cut_old, uint32_t* __restrict__ level)
{
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  level[p] = replan_open_level(cut_old[p]);
}

// The class of every plan and the three lists, ONE workgroup: plan p of chunk c sits in lane p - 1024 c, so a ballot per wave,
// the waves' counts in LDS and a running base per class give every plan its place in ascending plan order (no atomics: the
// order is that of the plan indices, whatever the schedule).  level[p] comes in as k_replan_open / k_replan_level left it and
// goes out as the rewind level L = min(that, cut).  lists: [0, n) KEPT, [n, 2n) REPAIRED, [2n, 3n) FRESH; counts[3].
//   KEPT      no logged one-ring reaches down to the cut, same target, same offset bits, a finalized field, not `unkeepable`
//   FRESH     otherwise, when f > 0, the cut is finite and positive and L / cut < f
//   REPAIRED  everything else
__global__ __launch_bounds__(kClassifyBlock) void k_replan_classify(const TilePlan* __restrict__ plans, uint32_t n, const uint32_t* __restrict__ old_target,
                                                                    const float* __restrict__ cut_old, uint32_t* __restrict__ level,
                                                                    uint32_t keepable, uint32_t unkeepable, double f, uint8_t* __restrict__ cls,
                                                                    float* __restrict__ ratio, uint32_t* __restrict__ lists, uint32_t* __restrict__ counts)
{
  __shared__ uint32_t s_w[3][kClassifyBlock / 64];
  __shared__ uint32_t s_base[3];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  if (tid < 3) s_base[tid] = 0u;
  __syncthreads();
  for (uint32_t p0 = 0; p0 < n; p0 += kClassifyBlock) {
    const uint32_t p = p0 + tid;
    const bool live = p < n;
    const uint32_t q = live ? p : 0u;                                 // (clamped: every load below is unconditional)
    const float cut = cut_old[q];
    const uint32_t raw = level[q], tg_old = old_target[q], tg_new = plans[q].target;
    const uint32_t lb = min(raw, f2u(cut));
    const bool finite = cut < inf_f() && cut > 0.0f;
    const double r = finite ? (double)u2f(lb) / (double)cut : (double)inf_f();
    const bool kept = raw == replan_open_level(cut) && tg_new == tg_old && keepable != 0u && p != unkeepable;
    const bool fresh = !kept && f > 0.0 && finite && r < f;
    const uint32_t c = kept ? kEachKept : fresh ? kEachFresh : kEachRepaired;
    const unsigned long long b0 = __ballot(live && c == kEachKept), b1 = __ballot(live && c == kEachRepaired), b2 = __ballot(live && c == kEachFresh);
    if (lane == 0) { s_w[0][w] = (uint32_t)__popcll(b0); s_w[1][w] = (uint32_t)__popcll(b1); s_w[2][w] = (uint32_t)__popcll(b2); }
    __syncthreads();
    uint32_t o0 = s_base[0], o1 = s_base[1], o2 = s_base[2];
    for (uint32_t k = 0; k < w; ++k) { o0 += s_w[0][k]; o1 += s_w[1][k]; o2 += s_w[2][k]; }
    if (live) {
      const uint32_t at = c == kEachKept ? o0 + (uint32_t)__popcll(b0 & below)
                        : c == kEachRepaired ? n + o1 + (uint32_t)__popcll(b1 & below) : 2u * n + o2 + (uint32_t)__popcll(b2 & below);
      lists[at] = p;
      cls[p] = (uint8_t)c; ratio[p] = (float)r; level[p] = lb;
    }
    __syncthreads();
    if (tid < 3) {
      uint32_t s = 0;
      for (int k = 0; k < kClassifyBlock / 64; ++k) s += s_w[tid][k];
      s_base[tid] += s;
    }
    __syncthreads();
  }
  if (tid < 3) counts[tid] = s_base[tid];
}

// What the gather reads and writes: the batch's records as fill_tile_records uploaded them, the lists, and the compacted
// arrays -- positions [0, nr) the REPAIRED plans, [nr, nr + nk) the KEPT ones, both in ascending plan order.
struct EachGather {
  const Plan* plans; const TilePlan* tplans; float* const* vecptrs; const uint32_t* level;
  const uint32_t* lists; const uint32_t* counts; uint32_t n;
  Plan* c_plans; TilePlan* c_tplans; float** c_vecptrs; uint32_t* c_level; ReplanCnt* c_cnt; TCtl* c_tctl; PlanResult* c_res;
};

// One wave per compacted position.  A REPAIRED plan gets its two records, its vector-map pointer, its level and zeroed
// counters; its control records move to the compacted pool (the host looks at the first nr of them between chunks of rounds)
// and start as k_replan_begin leaves them.  A KEPT plan gets its Plan record alone, for k_finish and k_count, and the control
// block k_dij_finalize would leave: nothing else of it is touched.  Result records start at zero.
__global__ __launch_bounds__(64) void k_replan_gather(EachGather G)
{
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  const uint32_t nk = G.counts[kEachKept], nr = G.counts[kEachRepaired];
  if (i >= nr + nk) return;                                           // (uniform over the wave)
  const bool rep = i < nr;
  const uint32_t p = min(G.lists[rep ? G.n + i : i - nr], G.n - 1u);
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(G.plans + p);
    uint32_t* dst = reinterpret_cast<uint32_t*>(G.c_plans + i);
    for (uint32_t k = lane; k < sizeof(Plan) / 4; k += 64) dst[k] = src[k];
  }
  if (rep) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(G.tplans + p);
    uint32_t* dst = reinterpret_cast<uint32_t*>(G.c_tplans + i);
    const uint32_t kc = (uint32_t)(offsetof(TilePlan, ctl) / 4);       // the control records move to the compacted pool
    const unsigned long long cp = (unsigned long long)(uintptr_t)(G.c_tctl + 2 * (size_t)i);
    for (uint32_t k = lane; k < sizeof(TilePlan) / 4; k += 64) dst[k] = k == kc ? (uint32_t)cp : k == kc + 1u ? (uint32_t)(cp >> 32) : src[k];
  }
  if (lane != 0) return;
  PlanResult z; memset(&z, 0, sizeof(z));
  G.c_res[i] = z;
  if (rep) {
    TCtl* const ctl = G.c_tctl + 2 * (size_t)i;
    TCtl c0; memset(&c0, 0, sizeof(c0));
    c0.it = -1; c0.done = 0; c0.thr = -inf_f(); c0.thr_prev = -inf_f();
    ctl[0] = c0; ctl[1] = c0;
    G.c_vecptrs[i] = G.vecptrs[p];
    G.c_level[i] = G.level[p];
    ReplanCnt zc; zc.kept = 0ull; zc.rewound = 0ull; zc.woken = 0u; zc.pad = 0u;
    G.c_cnt[i] = zc;
  } else {
    const Plan& P = G.plans[p];
    const uint32_t tg = min(P.target[0], P.V - 1u);
    const float dt = P.dist[tg];
    Ctl r; memset(&r, 0, sizeof(r));
    r.armed = dt < inf_f() ? 1u : 0u; r.goal_dist = goal_cut(dt, P.offset, tg).goal; r.thr = inf_f(); r.thr_fixed = inf_f(); r.done = 1u;
    P.ctl[0] = r; P.ctl[1] = r;
  }
}
