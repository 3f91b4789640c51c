// mnav_replan_each_capi.h -- the C ABI of the per-plan replan (include/mnav.h: mnav_replan_dijkstra_each, mnav_replan_each_stats;
// DESIGN.md §3.14) over the kernels of mnav_replan.h and mnav_replan_each.h, the tile rounds, the finalize pass and -- for the
// FRESH plans -- the engines of a Dijkstra call.  Included by mnav.hip inside its extern "C" block, after mnav_replan_capi.h.
#pragma once

// Default of the option replan_each_fresh_share: the share of FRESH plans above which the whole call plans afresh.  Measured on
// the 1M-vertex mesh (profiles/replan_each_perf.json): the per-plan call beat mnav_replan_dijkstra_batch 5 times over at shares
// of 0, 0.001 and 0.002 (64, 1 024, 7 168 plans; nearly every plan KEPT) and lost at every share from 0.016 up, where the
// REPAIRED plans' tile rounds cost more than planning the whole batch afresh; the crossings read between those rows are
// 0.0043, 0.0065 and 0.0059.  The smallest, rounded down: for 64 plans any FRESH plan sends the call to the fresh plan.
constexpr double kReplanEachFreshShare = 0.004;

static void replan_each_begin_stats(mnav_ctx* ctx, uint32_t reason, uint32_t log_len)
{
  mnav_ctx::Replan::Each& E = ctx->rp.each;
  E.reason = reason; E.whole_fresh = reason ? 1u : 0u; E.log_len = log_len;
  E.counts[0] = E.counts[1] = E.counts[2] = 0; E.tiles_woken = E.rounds = 0; E.fresh_engine = -1; E.kept = E.rewound = 0;
  E.cls.clear(); E.levels.clear();
  E.ms_classify = E.ms_rewind = E.ms_rounds = E.ms_finalize = E.ms_fresh = 0.f;
}

static int replan_each_reserve(mnav_ctx* ctx, uint32_t m)
{
  mnav_ctx::Replan::Each& E = ctx->rp.each;
  if (!E.have_ev) {
    for (auto& e : E.ev) HIPCHK(hipEventCreate(e.out()));
    E.have_ev = true;
  }
  if (m > E.cap) {
    E.cap = 0;
    if (alloc_group(E.d_cls, (size_t)m, E.d_ratio, 4 * (size_t)m, E.d_lists, 12 * (size_t)m, E.d_counts, 16, E.d_level, 4 * (size_t)m,
                    E.d_plans, sizeof(Plan) * (size_t)m, E.d_tplans, sizeof(TilePlan) * (size_t)m, E.d_vecptrs, sizeof(float*) * (size_t)m,
                    E.d_cnt, sizeof(ReplanCnt) * (size_t)m, E.d_tctl, 2 * sizeof(TCtl) * (size_t)m, E.d_res, sizeof(PlanResult) * (size_t)m) != hipSuccess) {
      ctx->err = "replan: out of device memory"; return -1;
    }
    E.cap = m;
  }
  return 0;
}

// ctx->slots[0, m) in the order `at` (position j takes the slot that stood at at[j]; `at` is a permutation of 0 .. m-1).  The
// handles move, no memory does; the control records of a slot are those of its position.
static void replan_each_permute_slots(mnav_ctx* ctx, uint32_t m, const std::vector<uint32_t>& at)
{
  std::vector<Slot> moved(m);
  for (uint32_t j = 0; j < m; ++j) moved[j] = std::move(ctx->slots[at[j]]);
  for (uint32_t j = 0; j < m; ++j) {
    ctx->slots[j] = std::move(moved[j]);
    ctx->slots[j].ctl = ctx->d_ctl_pool + 2 * j; ctx->slots[j].tctl = ctx->d_tctl_pool + 2 * j;
  }
}

// The per-plan repair of the m = n resident fields.  Returns 0 (done, *code set), -1 (error), 1 (cancelled) or 2 (the share
// policy: nothing was rewound yet, the caller plans the whole call afresh).
static int replan_each_repair(mnav_ctx* ctx, uint32_t n, const std::vector<uint32_t>& tg, double offset, uint32_t* codes_out, float* dist_out,
                              uint32_t* pred_out, uint32_t* path_out, uint32_t path_cap, uint32_t* path_len, uint32_t* code)
{
  mnav_ctx::Replan& R = ctx->rp;
  mnav_ctx::Replan::Each& E = R.each;
  const uint32_t m = n;
  RepairHead H;
  if (replan_repair_head(ctx, m, tg, offset, true, E.ev[0], H)) return -1;
  const std::vector<PlanIn>& in = H.in; const std::vector<uint32_t>& map = H.map;
  // a plan is kept as it is only when the record allows it (finalized field, vector map if one is wanted, the recorded
  // offset bits); never in slot 0 after an inflation wave took that slot's predecessors
  const bool keepable = ctx->res.may_keep(offset, ctx->want_vec);
  const double f = opt_set(ctx->opt.replan_fresh_below) ? ctx->opt.replan_fresh_below : kReplanFreshBelow;
  hipLaunchKernelGGL(k_replan_classify, dim3(1), dim3(kClassifyBlock), 0, ctx->stream, ctx->d_tplans, m, R.d_old_target, R.d_cut, R.d_level,
                     keepable ? 1u : 0u, ctx->res.slot0_lost() ? 0u : kNone, f, E.d_cls, E.d_ratio, E.d_lists, E.d_counts);
  EachGather G{};
  G.plans = ctx->d_plans; G.tplans = ctx->d_tplans; G.vecptrs = ctx->d_vecptrs; G.level = R.d_level; G.lists = E.d_lists; G.counts = E.d_counts; G.n = m;
  G.c_plans = E.d_plans; G.c_tplans = E.d_tplans; G.c_vecptrs = E.d_vecptrs; G.c_level = E.d_level; G.c_cnt = E.d_cnt; G.c_tctl = E.d_tctl; G.c_res = E.d_res;
  hipLaunchKernelGGL(k_replan_gather, dim3(m), dim3(64), 0, ctx->stream, G);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(E.ev[1], ctx->stream));
  E.cls.assign(m, 0); E.levels.assign(m, 0.f);
  std::vector<uint8_t> cls(m); std::vector<float> lv(m);
  uint32_t counts[4] = { 0, 0, 0, 0 };
  HIPCHK(hipMemcpyAsync(cls.data(), E.d_cls, (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(lv.data(), R.d_level, 4 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(counts, E.d_counts, 12, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));                          // (hp, tp, vecs, old_target are on the device now)
  const uint32_t nk = counts[kEachKept], nr = counts[kEachRepaired], nf = counts[kEachFresh];
  if (nk + nr + nf != m) { ctx->err = "replan: the classes do not add up"; return -1; }
  for (uint32_t k = 0; k < m; ++k) { E.cls[map[k]] = cls[k]; E.levels[map[k]] = lv[k]; }   // (the caller's order)
  E.counts[0] = nk; E.counts[1] = nr; E.counts[2] = nf;
  E.ms_classify = ev_ms(E.ev[0], E.ev[1]);
  const double share = opt_set(ctx->opt.replan_each_fresh_share) ? ctx->opt.replan_each_fresh_share : kReplanEachFreshShare;
  if (nf && (double)nf > share * (double)m) return 2;
  const bool warm = replan_takes_warm(ctx, nr);                       // the REPAIRED plans from their rewound fields on the tile-batch engine
  // the lists on the host: ascending device plan, as k_replan_classify wrote them
  std::vector<uint32_t> tail, fresh;                                  // tail: the REPAIRED plans, then the KEPT ones
  tail.reserve(nr + nk); fresh.reserve(nf);
  for (uint32_t k = 0; k < m; ++k) if (cls[k] == kEachRepaired) tail.push_back(k);
  for (uint32_t k = 0; k < m; ++k) if (cls[k] == kEachKept) tail.push_back(k);
  for (uint32_t k = 0; k < m; ++k) if (cls[k] == kEachFresh) fresh.push_back(k);
  replan_repair_begin(ctx, n, path_len);
  ctx->last_engine = 0;
  std::vector<uint32_t> codes(n, MNAV_SUCCESS);
  std::vector<PlanResult> res(m);                                     // per device plan, for the statistics of the whole call
  const TileTables T{ E.d_plans, E.d_tplans, E.d_tctl, E.d_res };
  HIPCHK(hipEventRecord(E.ev[2], ctx->stream));
  if (nr && !warm) {
    hipLaunchKernelGGL(k_replan_rewind, dim3(ctx->tiles_meta.ntiles ? ctx->tiles_meta.ntiles : 1u, nr), dim3(kTileBlock), 0, ctx->stream,
                       E.d_tplans, E.d_plans, E.d_level, E.d_cnt);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(E.ev[3], ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
  if (nr && !warm) {
    const int rc = run_tile_rounds(ctx, nr, &T);
    if (rc != 0) { (void)hipStreamSynchronize(ctx->stream); return rc < 0 ? -1 : 1; }
    E.rounds = ctx->stats.launches; E.ms_rounds = (float)ctx->ms_chunks;
    HIPCHK(hipEventRecord(E.ev[4], ctx->stream));
    launch_finalize(ctx, nr, 0, 0, &T);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(E.ev[5], ctx->stream));
  }
  HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
  // the compacted arrays: the REPAIRED plans the rounds finished, then the KEPT ones -- the KEPT ones alone when the repair runs
  // warm (first: the control records a KEPT plan's tail reads stand at its position, which the warm sub-batch takes over)
  const uint32_t skip = warm ? nr : 0u, nt = nr + nk - skip;
  if (nt) {
    std::vector<uint32_t> tmap(nt);
    for (uint32_t j = 0; j < nt; ++j) tmap[j] = map[tail[skip + j]];
    const TailSub sub{ E.d_plans.get() + skip, E.d_res.get() + skip, E.d_vecptrs.get() + skip, nr - skip, tail.data() + skip };
    if (dijkstra_tail(ctx, nt, 0, tmap, codes, dist_out, pred_out, path_out, path_cap, path_len, nullptr, ctx->want_vec, &sub)) return -1;
    for (uint32_t j = 0; j < nt; ++j) res[tail[skip + j]] = ctx->h_res[j];
  }
  if (warm) {
    const std::vector<uint32_t> who(tail.begin(), tail.begin() + nr);
    ReplanCnt tot{};
    const int rc = replan_warm_run(ctx, m, in, who, lv, map, offset, codes, dist_out, pred_out, path_out, path_cap, path_len, &res, &tot);
    if (rc != 0) return rc;
    E.kept = tot.kept; E.rewound = tot.rewound; E.tiles_woken = tot.woken;
    E.rounds = R.warm.iters; E.ms_rewind = R.warm.ms_warm; E.ms_rounds = R.warm.ms_engine; E.ms_finalize = R.warm.ms_finalize;
  } else
  if (nr) {
    std::vector<ReplanCnt> cnt(nr);
    HIPCHK(hipMemcpy(cnt.data(), E.d_cnt, sizeof(ReplanCnt) * (size_t)nr, hipMemcpyDeviceToHost));
    for (uint32_t j = 0; j < nr; ++j) { E.kept += cnt[j].kept; E.rewound += cnt[j].rewound; E.tiles_woken += cnt[j].woken; }
    E.ms_rewind = ev_ms(E.ev[2], E.ev[3]); E.ms_finalize = ev_ms(E.ev[4], E.ev[5]);
  }
  int sub_engine = -1;
  if (nf) {
    // the FRESH plans as a batch of their own, in the first nf slots, on the engine `auto` picks for their number
    int engine = dijkstra_auto_engine(ctx, nf);
    if (engine == 5 && nf > 65535u) engine = 0;
    std::vector<PlanIn> fin(nf); std::vector<uint32_t> who = fresh;   // who: sub-batch position -> device plan of this call
    for (uint32_t j = 0; j < nf; ++j) fin[j] = in[fresh[j]];
    if (dijkstra_order(ctx, engine, fin, who)) return -1;
    std::vector<uint32_t> at(m), back(m), fmap(nf);
    {
      std::vector<uint8_t> taken(m, 0);
      for (uint32_t j = 0; j < nf; ++j) { at[j] = who[j]; taken[who[j]] = 1; fmap[j] = map[who[j]]; }
      uint32_t j = nf;
      for (uint32_t k = 0; k < m; ++k) if (!taken[k]) at[j++] = k;
      for (uint32_t q = 0; q < m; ++q) back[at[q]] = q;
    }
    const auto t0 = std::chrono::steady_clock::now();
    replan_each_permute_slots(ctx, m, at);
    int rc = dijkstra_dispatch(ctx, nf, fin, offset, true, &engine);
    if (rc == 0) {
      ctx->last_engine = engine;
      if (dijkstra_tail(ctx, nf, engine, fmap, codes, dist_out, pred_out, path_out, path_cap, path_len, nullptr, ctx->want_vec)) rc = -1;
    }
    if (rc == 0) for (uint32_t j = 0; j < nf; ++j) res[who[j]] = ctx->h_res[j];
    replan_each_permute_slots(ctx, m, back);
    ctx->last_engine = 0; ctx->tb.count_pending = false; ctx->tb_args_valid = false;
    if (rc != 0) return rc < 0 ? -1 : 1;
    E.ms_fresh = (float)(1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    sub_engine = engine + ((engine == 5 && ctx->tb.kernel == 1) ? 16 : 0);
  }
  E.fresh_engine = sub_engine;
  // the whole call's results in device-plan order, as the statistics and the lazy readers expect them
  for (uint32_t k = 0; k < m; ++k) ctx->h_res[k] = res[k];
  finish_stats(ctx, m, false);
  R.each_engines = 256 + (warm ? 512 + (R.warm.kernel == 1 ? 1024 : 0) : nr ? 128 : 0) + (sub_engine >= 0 ? sub_engine : 127);
  R.levels = E.levels; R.kept = E.kept; R.rewound = E.rewound; R.tiles_woken = E.tiles_woken; R.rounds = E.rounds;
  R.ms_level = E.ms_classify; R.ms_rewind = E.ms_rewind; R.ms_rounds = E.ms_rounds; R.ms_finalize = E.ms_finalize;
  replan_repair_commit(ctx, tg, offset, codes, codes_out, code);
  return 0;
}

uint32_t mnav_replan_dijkstra_each(mnav_ctx* ctx, uint32_t n, const uint32_t* targets, double goal_dist_offset, uint32_t* codes_out, float* dist_out,
                                   uint32_t* pred_out, uint32_t* path_out, uint32_t path_cap, uint32_t* path_len)
{
  return replan_call(ctx, n, targets, goal_dist_offset, codes_out, dist_out, pred_out, path_out, path_cap, path_len, true);
}

int mnav_replan_each_stats(const mnav_ctx* ctx, uint32_t* reason, uint32_t* whole_fresh, uint32_t* log_len, uint8_t* classes_out, float* levels_out,
                           uint32_t* counts, uint64_t* kept, uint64_t* rewound, uint32_t* tiles_woken, uint32_t* rounds, int32_t* fresh_engine,
                           float* ms)
{
  if (!ctx) return -1;
  const mnav_ctx::Replan::Each& E = ctx->rp.each;
  if (reason) *reason = E.reason;
  if (whole_fresh) *whole_fresh = E.whole_fresh;
  if (log_len) *log_len = E.log_len;
  if (classes_out) for (size_t i = 0; i < E.cls.size(); ++i) classes_out[i] = E.cls[i];
  if (levels_out) for (size_t i = 0; i < E.levels.size(); ++i) levels_out[i] = E.levels[i];
  if (counts) for (int k = 0; k < 3; ++k) counts[k] = E.counts[k];
  if (kept) *kept = E.kept;
  if (rewound) *rewound = E.rewound;
  if (tiles_woken) *tiles_woken = E.tiles_woken;
  if (rounds) *rounds = E.rounds;
  if (fresh_engine) *fresh_engine = E.fresh_engine;
  if (ms) { ms[0] = E.ms_classify; ms[1] = E.ms_rewind; ms[2] = E.ms_rounds; ms[3] = E.ms_finalize; ms[4] = E.ms_fresh; }
  return 0;
}
