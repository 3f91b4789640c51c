// mnav_replan_capi.h -- the C ABI of the replan (include/mnav.h: mnav_replan_dijkstra_batch, mnav_replan_plans, mnav_replan_stats) over the
// kernels of mnav_replan.h, the tile rounds and the finalize pass.  Included by mnav.hip inside its extern "C" block, after
// dijkstra_impl (the fresh path) and its helpers.
#pragma once

// Default of the option replan_fresh_below.  Measured on the 1M-vertex mesh (profiles/replan_perf.json): below a smallest
// L / cut_old of 0.25 the fresh plan won for one plan and for 64; one plan alone crosses at 0.50, 64 plans between 0.25 and 0.38.
constexpr double kReplanFreshBelow = 0.25;

static int replan_reserve(mnav_ctx* ctx, uint32_t m)
{
  mnav_ctx::Replan& R = ctx->rp;
  if (!R.have_ev) {
    for (auto& e : R.ev) HIPCHK(hipEventCreate(e.out()));
    R.have_ev = true;
  }
  if (m > R.cap) {
    R.cap = 0;
    if (alloc_group(R.d_level, 4 * (size_t)m, R.d_old_target, 4 * (size_t)m, R.d_cut, 4 * (size_t)m, R.d_cnt, sizeof(ReplanCnt) * (size_t)m) != hipSuccess) {
      ctx->err = "replan: out of device memory"; return -1;
    }
    R.cap = m;
  }
  return 0;
}

// Default of the option replan_warm_min_plans: in automatic mode (replan_repair_engine unset) the repaired plans of a replan
// call start the tile-batch engine from their rewound fields (k_tb_warm) when there are at least this many of them; fewer are
// finished on the tile rounds.  Never below 161: under that a fresh plan does not take the tile-batch engine either
// (dijkstra_auto_engine).  Measured on the 1M-vertex mesh (profiles/replan_each_perf.json, repair_engine_cases):
// the warm start lost to the rounds at 2, 9, 35 and 63 repaired plans, won at 18, 43 and 64 by 2 to 15 % and from 299 on by 2.1 to
// 9.3 times, with nothing measured between 64 and 299.  299 is the smallest measured count with a win that no measured loss
// stands next to.
constexpr uint32_t kReplanWarmMinPlans = 299u;
static_assert(kReplanWarmMinPlans >= 161u, "under 161 plans a fresh plan does not take the tile-batch engine either");

static void replan_each_permute_slots(mnav_ctx* ctx, uint32_t m, const std::vector<uint32_t>& at);   // (mnav_replan_each_capi.h)

static void replan_warm_begin_stats(mnav_ctx* ctx)
{
  mnav_ctx::Replan::Warm& Wm = ctx->rp.warm;
  Wm.plans = Wm.kernel = Wm.iters = Wm.fallback = 0; Wm.woken = Wm.words = 0; Wm.live = false;
  Wm.ms_warm = Wm.ms_engine = Wm.ms_finalize = 0.f;
}

// Whether the nr repaired plans of a replan call run warm on the tile-batch engine.  Called before anything is rewound.  An
// engine that cannot be used is a fall-back to the tile rounds, recorded in the statistics, never an error: 1 = more than
// 65535 plans, 2 = the engine's tables or its batch state could not be built or allocated next to the resident outputs.
static bool replan_takes_warm(mnav_ctx* ctx, uint32_t nr)
{
  mnav_ctx::Replan::Warm& Wm = ctx->rp.warm;
  if (!nr) return false;
  const int e = opt_set(ctx->opt.replan_repair_engine) ? (int)ctx->opt.replan_repair_engine : -1;
  if (e == 0) return false;
  if (e != 5 && nr < opt_u32(ctx->opt.replan_warm_min_plans, kReplanWarmMinPlans)) return false;
  if (nr > 65535u) { Wm.fallback = 1; return false; }                 // (plan ids are 16 bits in the tile-batch buckets)
  bool ok = tb_build(ctx) == 0 && tb_ensure_batch(ctx, nr) == 0;
  if (ok && nr > Wm.cap) {
    Wm.cap = 0;
    ok = alloc_group(Wm.d_level, 4 * (size_t)nr, Wm.d_dist, sizeof(float*) * (size_t)nr, Wm.d_cnt, sizeof(ReplanCnt) * (size_t)nr) == hipSuccess;
    if (ok) Wm.cap = nr;
  }
  if (!ok) { (void)hipGetLastError(); ctx->err.clear(); Wm.fallback = 2; return false; }
  return true;
}

// The warm repair of the device plans `who` of a call of m plans: they move to the first slots in the order the tile-batch
// engine wants them (dijkstra_order), levels and potentials follow that order, the engine starts from k_tb_warm, its finalize
// pass and the tail of a Dijkstra call write the outputs, and the slots move back.  in, lv (rewind levels), map: per device
// plan of the call.  res (optional): the result record of every plan served, per device plan.  Returns 0, -1 or 1 (cancelled).
static int replan_warm_run(mnav_ctx* ctx, uint32_t m, const std::vector<PlanIn>& in, std::vector<uint32_t> who, const std::vector<float>& lv,
                           const std::vector<uint32_t>& map, double offset, std::vector<uint32_t>& codes, float* dist_out, uint32_t* pred_out,
                           uint32_t* path_out, uint32_t path_cap, uint32_t* path_len, std::vector<PlanResult>* res, ReplanCnt* total)
{
  mnav_ctx::Replan::Warm& Wm = ctx->rp.warm;
  const uint32_t nr = (uint32_t)who.size();
  std::vector<PlanIn> win(nr);
  for (uint32_t j = 0; j < nr; ++j) win[j] = in[who[j]];
  if (dijkstra_order(ctx, 5, win, who)) return -1;
  std::vector<uint32_t> at(m), back(m), wmap(nr);
  {
    std::vector<uint8_t> taken(m, 0);
    for (uint32_t j = 0; j < nr; ++j) { at[j] = who[j]; taken[who[j]] = 1; wmap[j] = map[who[j]]; }
    uint32_t j = nr;
    for (uint32_t k = 0; k < m; ++k) if (!taken[k]) at[j++] = k;
    for (uint32_t q = 0; q < m; ++q) back[at[q]] = q;
  }
  replan_each_permute_slots(ctx, m, at);
  int rc = 0;
  {
    std::vector<float> wl(nr); std::vector<const float*> wd(nr);
    for (uint32_t j = 0; j < nr; ++j) { wl[j] = lv[who[j]]; wd[j] = ctx->slots[j].dist.get(); }
    if (hipMemcpyAsync(Wm.d_level, wl.data(), 4 * (size_t)nr, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(Wm.d_dist, wd.data(), sizeof(float*) * (size_t)nr, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->err = "replan: upload of the warm start's arrays failed"; rc = -1; }
  }
  if (rc == 0) {
    const TbWarmIn w{ Wm.d_level, Wm.d_dist, Wm.d_cnt };
    rc = run_dijkstra_tb(ctx, nr, win, offset, &w);
    if (rc != 0) (void)hipStreamSynchronize(ctx->stream);             // nothing of a failed / cancelled call stays in flight
  }
  if (rc == 0) {
    ctx->last_engine = 5;
    if (dijkstra_tail(ctx, nr, 5, wmap, codes, dist_out, pred_out, path_out, path_cap, path_len, nullptr, ctx->want_vec)) rc = -1;
  }
  if (rc == 0 && res) for (uint32_t j = 0; j < nr; ++j) (*res)[who[j]] = ctx->h_res[j];
  replan_each_permute_slots(ctx, m, back);
  ctx->last_engine = 0; ctx->tb.count_pending = false; ctx->tb_args_valid = false;   // (the engine's arguments name the slots in sub-batch order)
  if (rc != 0) return rc < 0 ? -1 : 1;
  std::vector<ReplanCnt> cnt(nr);
  HIPCHK(hipMemcpy(cnt.data(), Wm.d_cnt, sizeof(ReplanCnt) * (size_t)nr, hipMemcpyDeviceToHost));
  total->kept = total->rewound = 0; total->woken = 0;
  Wm.woken = 0;
  for (uint32_t j = 0; j < nr; ++j) { total->kept += cnt[j].kept; total->rewound += cnt[j].rewound; Wm.woken += cnt[j].woken; }
  total->woken = (uint32_t)std::min<uint64_t>(Wm.woken, 0xFFFFFFFFull);
  Wm.plans = nr; Wm.kernel = (uint32_t)ctx->tb.kernel; Wm.iters = ctx->tb.last.iters; Wm.words = ctx->tb.S * (uint64_t)nr;
  Wm.ms_warm = ctx->tb.ms_warm; Wm.ms_engine = (float)ctx->ms_chunks; Wm.ms_finalize = ctx->tb.ms_warm_fin; Wm.live = true;
  return 0;
}

static int replan_each_reserve(mnav_ctx* ctx, uint32_t m);            // (mnav_replan_each_capi.h)

// What both repairs of the m = n recorded fields start with.  in: the plans towards the new robot vertices in their recorded
// slots; map: device plan -> caller's index.  The other vectors are sources of copies in flight: the whole struct lives
// until the repair's first synchronisation.
struct RepairHead {
  std::vector<PlanIn> in; std::vector<uint32_t> map, old_target;
  std::vector<Plan> hp; std::vector<TilePlan> tp; std::vector<float*> vecs;
};

// The head of a repair: the parameters of the running call, every reservation, the tile records, the old targets on the
// device and, behind the event ev_begin, the rewind levels (k_replan_begin, for the per-plan repair k_replan_open,
// k_replan_level over the change log).  ev_begin may be created by the reservations.  The fields are as they were when it returns.
static int replan_repair_head(mnav_ctx* ctx, uint32_t m, const std::vector<uint32_t>& tg, double offset, bool each, const Event& ev_begin, RepairHead& H)
{
  mnav_ctx::Replan& R = ctx->rp;
  const Resident& L = ctx->res;
  H.in.resize(m); H.map.resize(m); H.old_target.resize(m);
  for (uint32_t i = 0; i < m; ++i) {
    const uint32_t k = L.recorded_slot(i);
    H.in[k] = vertex_plan(L.seeds()[i], tg[i]); H.map[k] = i; H.old_target[k] = L.targets()[i];
  }
  ctx->want_vec = ctx->resident_vecmap;
  ctx->lazy_paths = false;                                            // the finalize pass always runs: predecessors and vector maps are re-derived
  if (replan_reserve(ctx, m) || (each && replan_each_reserve(ctx, m))) return -1;
  if (materialize(ctx, false, L.cost_limit())) return -1;
  if (ensure_slots(ctx, m, false, false, ctx->want_vec)) return -1;
  if (ensure_paths(ctx, m)) return -1;
  if (ensure_tile_state(ctx, m)) return -1;
  if (tile_weights(ctx)) return -1;
  (void)hipEventRecord(ctx->ev[0], ctx->stream);
  if (fill_tile_records(ctx, m, H.in, offset, H.hp, H.tp, H.vecs)) return -1;
  HIPCHK(hipMemcpyAsync(R.d_old_target, H.old_target.data(), 4 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  HIPCHK(hipEventRecord(ev_begin, ctx->stream));
  const uint32_t gm = (m + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_replan_begin, dim3(gm), dim3(kBlock), 0, ctx->stream, ctx->d_tplans, m, R.d_old_target, L.offset(), R.d_level, R.d_cut, R.d_cnt);
  if (each) hipLaunchKernelGGL(k_replan_open, dim3(gm), dim3(kBlock), 0, ctx->stream, m, R.d_cut, R.d_level);
  if (R.len)
    hipLaunchKernelGGL(k_replan_level, dim3((R.len + kBlock - 1) / kBlock, m), dim3(kBlock), 0, ctx->stream, ctx->d_tplans, R.log, R.len,
                       ctx->d_row_ptr, ctx->d_nbr_u, R.d_level);
  return 0;
}

// From here on a repair changes the fields: the record follows, the outputs count again once the repair commits.
static void replan_repair_begin(mnav_ctx* ctx, uint32_t n, uint32_t* path_len)
{
  ctx->res.repair_begin();
  resident_outputs_begin(ctx);
  for (uint32_t i = 0; i < n; ++i) if (path_len) path_len[i] = 0;
}

// The repair went through: the record takes the new robot vertices and the offset, the caller its codes.
static void replan_repair_commit(mnav_ctx* ctx, const std::vector<uint32_t>& tg, double offset, const std::vector<uint32_t>& codes, uint32_t* codes_out, uint32_t* code)
{
  ctx->res.repair_commit(tg, offset, ctx->want_vec);
  resident_outputs_commit(ctx);
  uint32_t worst = MNAV_SUCCESS;
  for (size_t i = 0; i < codes.size(); ++i) {
    if (codes_out) codes_out[i] = codes[i];
    if (codes[i] != MNAV_SUCCESS && worst == MNAV_SUCCESS) worst = codes[i];
  }
  *code = worst;
}

// The repair of the m = n resident fields.  tg: the new robot vertices in the caller's order.  Returns 0 (done, *code set),
// -1 (error), 1 (cancelled) or 2 (policy: nothing was rewound yet, the caller plans afresh).
static int replan_repair(mnav_ctx* ctx, uint32_t n, const std::vector<uint32_t>& tg, double offset, uint32_t* codes_out, float* dist_out,
                         uint32_t* pred_out, uint32_t* path_out, uint32_t path_cap, uint32_t* path_len, uint32_t* code)
{
  mnav_ctx::Replan& R = ctx->rp;
  const uint32_t m = n;
  RepairHead H;
  if (replan_repair_head(ctx, m, tg, offset, false, R.ev[0], H)) return -1;
  const std::vector<PlanIn>& in = H.in; const std::vector<uint32_t>& map = H.map;
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(R.ev[1], ctx->stream));
  std::vector<float> cut(m);
  R.levels.assign(m, 0.f);
  HIPCHK(hipMemcpyAsync(R.levels.data(), R.d_level, 4 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(cut.data(), R.d_cut, 4 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));                          // (hp, tp, vecs, old_target are on the device now)
  const double f = opt_set(ctx->opt.replan_fresh_below) ? ctx->opt.replan_fresh_below : kReplanFreshBelow;
  if (f > 0.0) {
    double share = INFINITY;                                          // plans with an infinite old cut do not vote
    for (uint32_t k = 0; k < m; ++k) if (cut[k] < INFINITY && cut[k] > 0.f) share = std::min(share, (double)R.levels[k] / (double)cut[k]);
    if (share < f) return 2;
  }
  const bool warm = replan_takes_warm(ctx, m);                        // all m plans from their rewound fields on the tile-batch engine
  replan_repair_begin(ctx, n, path_len);
  std::vector<uint32_t> codes(n, MNAV_SUCCESS);
  if (warm) {
    std::vector<uint32_t> who(m);
    std::iota(who.begin(), who.end(), 0u);
    ReplanCnt tot{};
    const int rc = replan_warm_run(ctx, m, in, who, R.levels, map, offset, codes, dist_out, pred_out, path_out, path_cap, path_len, nullptr, &tot);
    if (rc != 0) return rc;
    ctx->last_engine = 5;
    R.kept = tot.kept; R.rewound = tot.rewound; R.tiles_woken = tot.woken;
  } else {
  hipLaunchKernelGGL(k_replan_rewind, dim3(ctx->tiles_meta.ntiles ? ctx->tiles_meta.ntiles : 1u, m), dim3(kTileBlock), 0, ctx->stream,
                     ctx->d_tplans, ctx->d_plans, R.d_level, R.d_cnt);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(R.ev[2], ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
  const int rc = run_tile_rounds(ctx, m);
  if (rc != 0) { (void)hipStreamSynchronize(ctx->stream); return rc < 0 ? -1 : 1; }
  HIPCHK(hipEventRecord(R.ev[3], ctx->stream));
  launch_finalize(ctx, m);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(R.ev[4], ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
  ctx->last_engine = 0;
  if (dijkstra_tail(ctx, m, 0, map, codes, dist_out, pred_out, path_out, path_cap, path_len, nullptr, ctx->want_vec)) return -1;
  std::vector<ReplanCnt> cnt(m);
  HIPCHK(hipMemcpy(cnt.data(), R.d_cnt, sizeof(ReplanCnt) * (size_t)m, hipMemcpyDeviceToHost));
  R.kept = R.rewound = 0; R.tiles_woken = 0;
  for (uint32_t k = 0; k < m; ++k) { R.kept += cnt[k].kept; R.rewound += cnt[k].rewound; R.tiles_woken += cnt[k].woken; }
  }
  {
    std::vector<float> lv(m);                                         // levels in the caller's order
    for (uint32_t k = 0; k < m; ++k) lv[map[k]] = R.levels[k];
    R.levels.swap(lv);
  }
  R.ms_level = ev_ms(R.ev[0], R.ev[1]);
  if (warm) { R.rounds = R.warm.iters; R.ms_rewind = R.warm.ms_warm; R.ms_rounds = R.warm.ms_engine; R.ms_finalize = R.warm.ms_finalize; }
  else { R.rounds = ctx->stats.launches; R.ms_rewind = ev_ms(R.ev[1], R.ev[2]); R.ms_rounds = (float)ctx->ms_chunks; R.ms_finalize = ev_ms(R.ev[3], R.ev[4]); }
  replan_repair_commit(ctx, tg, offset, codes, codes_out, code);
  return 0;
}

// mnav_replan_each_capi.h: the repair plan by plan; 2 = its share policy sends the whole call to a fresh plan
static int replan_each_repair(mnav_ctx* ctx, uint32_t n, const std::vector<uint32_t>& tg, double offset, uint32_t* codes_out, float* dist_out,
                              uint32_t* pred_out, uint32_t* path_out, uint32_t path_cap, uint32_t* path_len, uint32_t* code);
static void replan_each_begin_stats(mnav_ctx* ctx, uint32_t reason, uint32_t log_len);

// Both replan entry points: the refusals, the whole-call reasons and the fresh plan they end in are the same; `each` picks
// the repair.
static uint32_t replan_call(mnav_ctx* ctx, uint32_t n, const uint32_t* targets, double goal_dist_offset, uint32_t* codes_out, float* dist_out,
                            uint32_t* pred_out, uint32_t* path_out, uint32_t path_cap, uint32_t* path_len, bool each)
{
  if (!ctx) return MNAV_INTERNAL_ERROR;
  mnav_ctx::Replan& R = ctx->rp;
  Resident& L = ctx->res;
  // refusals: outputs, change log and replan state stay as they are
  ctx->err.clear();
  if (!ctx->have_mesh) { ctx->err = "mnav_upload_mesh has not been called"; return MNAV_INTERNAL_ERROR; }
  if (goal_dist_offset != goal_dist_offset) { ctx->err = "goal_dist_offset is NaN"; return MNAV_INTERNAL_ERROR; }
  if (!L.has_recorded_call()) { ctx->err = "replan: no Dijkstra call to bring up to date (mnav_plan_dijkstra* first)"; return MNAV_INTERNAL_ERROR; }
  if (n != L.seeds().size()) { ctx->err = "replan: n differs from the last Dijkstra call"; return MNAV_INTERNAL_ERROR; }
  if (check_ready(ctx)) return MNAV_INTERNAL_ERROR;
  if (n == 0) return MNAV_SUCCESS;
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MNAV_INTERNAL_ERROR; }
  cancel_reset(ctx);
  const std::vector<uint32_t> seeds = L.seeds();
  const std::vector<uint32_t> tg = targets ? std::vector<uint32_t>(targets, targets + n) : L.targets();
  const uint32_t log_len = R.len;
  const double cost_limit = L.cost_limit();
  const uint32_t reason = L.replan_reason(n, tg, ctx->V, ctx->slots.size(), R.all);
  R.reason = reason; R.stat_log_len = log_len; R.kept = R.rewound = 0; R.tiles_woken = R.rounds = 0; R.levels.clear();
  R.ms_level = R.ms_rewind = R.ms_rounds = R.ms_finalize = 0.f;
  replan_warm_begin_stats(ctx);
  if (each) replan_each_begin_stats(ctx, reason, log_len);
  if (reason == 0) {
    uint32_t code = MNAV_INTERNAL_ERROR;
    const int rc = each ? replan_each_repair(ctx, n, tg, goal_dist_offset, codes_out, dist_out, pred_out, path_out, path_cap, path_len, &code)
                        : replan_repair(ctx, n, tg, goal_dist_offset, codes_out, dist_out, pred_out, path_out, path_cap, path_len, &code);
    if (rc == 0) return code;
    if (rc == 1) {                                                    // cancelled between two chunks of rounds: the fields are half rewound
      L.call_failed();
      for (uint32_t i = 0; i < n; ++i) if (codes_out) codes_out[i] = MNAV_CANCELED;
      return MNAV_CANCELED;
    }
    if (rc < 0) { L.call_failed(); (void)hipStreamSynchronize(ctx->stream); return MNAV_INTERNAL_ERROR; }
    R.reason = 4; R.levels.clear(); R.warm.fallback = 0;              // policy: plan afresh
    if (each) { R.each.reason = 4; R.each.whole_fresh = 1; }
  }
  // a fresh plan from the recorded seeds, finalize pass included: always a correct answer
  const bool lazy = ctx->allow_lazy_paths;
  ctx->allow_lazy_paths = false;
  const uint32_t rc = dijkstra_impl(ctx, n, seeds.data(), tg.data(), goal_dist_offset, cost_limit, codes_out, dist_out, pred_out, path_out, path_cap,
                                    path_len, nullptr, false);
  ctx->allow_lazy_paths = lazy;
  return rc;
}

uint32_t mnav_replan_dijkstra_batch(mnav_ctx* ctx, uint32_t n, const uint32_t* targets, double goal_dist_offset, uint32_t* codes_out, float* dist_out,
                                    uint32_t* pred_out, uint32_t* path_out, uint32_t path_cap, uint32_t* path_len)
{
  return replan_call(ctx, n, targets, goal_dist_offset, codes_out, dist_out, pred_out, path_out, path_cap, path_len, false);
}

uint32_t mnav_replan_plans(const mnav_ctx* ctx) { return ctx && ctx->res.has_recorded_call() ? (uint32_t)ctx->res.seeds().size() : 0u; }

int mnav_replan_stats(const mnav_ctx* ctx, uint32_t* reason, uint32_t* log_len, float* levels_out, uint64_t* kept, uint64_t* rewound,
                      uint32_t* tiles_woken, uint32_t* rounds, float* ms_level, float* ms_rewind, float* ms_rounds, float* ms_finalize)
{
  if (!ctx) return -1;
  const mnav_ctx::Replan& R = ctx->rp;
  if (reason) *reason = R.reason;
  if (log_len) *log_len = R.stat_log_len;
  if (levels_out) for (size_t i = 0; i < R.levels.size(); ++i) levels_out[i] = R.levels[i];
  if (kept) *kept = R.kept;
  if (rewound) *rewound = R.rewound;
  if (tiles_woken) *tiles_woken = R.tiles_woken;
  if (rounds) *rounds = R.rounds;
  if (ms_level) *ms_level = R.ms_level;
  if (ms_rewind) *ms_rewind = R.ms_rewind;
  if (ms_rounds) *ms_rounds = R.ms_rounds;
  if (ms_finalize) *ms_finalize = R.ms_finalize;
  return 0;
}

int mnav_replan_warm_stats(const mnav_ctx* ctx, uint32_t* plans, uint32_t* kernel, uint32_t* iterations, uint64_t* pairs_woken, uint64_t* words,
                           float* ms, uint32_t* fallback, uint32_t* live)
{
  if (!ctx) return -1;
  const mnav_ctx::Replan::Warm& Wm = ctx->rp.warm;
  if (plans) *plans = Wm.plans;
  if (kernel) *kernel = Wm.kernel;
  if (iterations) *iterations = Wm.iters;
  if (pairs_woken) *pairs_woken = Wm.woken;
  if (words) *words = Wm.words;
  if (ms) { ms[0] = Wm.ms_warm; ms[1] = Wm.ms_engine; ms[2] = Wm.ms_finalize; }
  if (fallback) *fallback = Wm.fallback;
  if (live) *live = Wm.live ? 1u : 0u;
  return 0;
}
