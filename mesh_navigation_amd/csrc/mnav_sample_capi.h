// mnav_sample_capi.h -- the C ABI of the sampled rollouts (include/mnav.h: mnav_follow_sample, mnav_sample_stats) over the
// kernels of mnav_sample.h.  Included by mnav.hip inside its extern "C" block, after mnav_rollout_capi.h: the argument
// checks, the staging, the rollout's buffers, the index build and the block loop are the rollout's own.  The statistics are
// kept apart (ctx->smp_rec): a call leaves what every other *_stats tells alone.
#pragma once

static_assert(sizeof(mnav_smp::Cand) == sizeof(double) * mnav_smp::kCandDoubles, "a candidate is four doubles");

// what the rows need beside the staging and the rollout's buffers: n robots, rows = n * K candidate rows, K candidates
static int sample_reserve(mnav_ctx* ctx, size_t n, size_t rows, size_t K, size_t n_slots)
{
  mnav_smp::Dev& D = ctx->smp;
  const char* oom = "sample: out of device memory";
  if (!D.have_ev) {
    for (auto& e : D.ev) HIPCHK(hipEventCreate(e.out()));
    D.have_ev = true;
  }
  if (!D.cnt) HIPCHK(D.cnt.alloc(sizeof(uint32_t) * mnav_smp::kPickCounters));
  if (n > D.cap) {
    D.cap = 0;
    if (alloc_group(D.in_pos, 12 * n, D.in_dir, 12 * n, D.in_face, 4 * n, D.in_slot, 4 * n, D.in_seed, 4 * n, D.best_k, 4 * n, D.n_feasible, 4 * n, D.best_score, 8 * n,
                    D.best_cmd, 16 * n) != hipSuccess) { ctx->err = oom; return -1; }
    D.cap = n;
  }
  if (rows > D.rows_cap) {
    D.rows_cap = 0;
    if (alloc_group(D.pot, 4 * rows, D.lethal, rows, D.cmd0, 16 * rows, D.score, 8 * rows) != hipSuccess) { ctx->err = oom; return -1; }
    D.rows_cap = rows;
  }
  if (K > D.table_cap) {
    D.table_cap = 0;
    if (D.table.alloc(sizeof(mnav_smp::Cand) * K) != hipSuccess) { ctx->err = oom; return -1; }
    D.table_cap = K;
  }
  if (n_slots > D.slots_cap) {
    D.slots_cap = 0;
    HIPCHK(D.pots.alloc(sizeof(const float*) * n_slots));
    D.slots_cap = n_slots;
  }
  return 0;
}

// The argument checks of a sampled rollout beside the rollout's, all on the host: -1 with ctx->err set, or 0 and pots[s] = the
// resident potential of every slot a robot uses.
static int sample_check(mnav_ctx* ctx, uint32_t n, const uint32_t* slots, const mnav_follow_config* config, const mnav_rollout_config* rollout, uint32_t K,
                        const double* table, const mnav_sample_config* sample, std::vector<const float*>& pots)
{
  if (!K || !table) { ctx->err = "sample: no candidates (n_candidates = 0 or a null table)"; return -1; }
  if (!sample) { ctx->err = "sample: null argument"; return -1; }
  if (sample->flags) { ctx->err = "sample: the flags of the sample config are reserved and must be 0"; return -1; }
  for (const double w : { sample->w_potential, sample->w_cost, sample->w_time })
    if (!(w >= 0.0) || !std::isfinite(w)) { ctx->err = "sample: a weight is negative or not finite"; return -1; }
  if (std::isnan(sample->lethal_cost)) { ctx->err = "sample: lethal_cost is NaN"; return -1; }
  if ((uint64_t)n * K > mnav_smp::kMaxRows) { ctx->err = "sample: more than 2^28 candidate rows (n * n_candidates)"; return -1; }
  // the restated sinf / cosf are the host libm's on (-120, 120) only: |u_ang| <= |ang_gain| * (the rollout's bound on |R.ang|) + |ang_bias|
  const double follower = std::fabs(config->max_ang_velocity) * std::fmax(1.0, std::fabs(config->ang_vel_factor));
  double turn = 0.0;
  for (size_t k = 0; k < (size_t)mnav_smp::kCandDoubles * K; ++k)
    if (!std::isfinite(table[k])) { ctx->err = "sample: a gain or bias is not finite"; return -1; }
  for (uint32_t k = 0; k < K; ++k) turn = std::fmax(turn, std::fabs(table[4 * (size_t)k + 2]) * follower + std::fabs(table[4 * (size_t)k + 3]));
  if (!(turn * rollout->dt < 100.0)) { ctx->err = "sample: (|ang_gain| * max_ang_velocity * max(1, ang_vel_factor) + |ang_bias|) * dt must stay below 100 rad per tick"; return -1; }
  const size_t n_slots = ctx->res.plans();
  pots.assign(n_slots ? n_slots : 1, nullptr);
  for (uint32_t i = 0; i < n; ++i) {                                  // (follow_check has seen every slot)
    const uint32_t s = slots[i];
    if (pots[s]) continue;
    pots[s] = static_cast<const float*>(mnav_device_output(ctx, s, 0));
    if (!pots[s]) { ctx->err = "sample: potential of slot " + std::to_string(s) + " not resident"; return -1; }
  }
  return 0;
}

int mnav_follow_sample(mnav_ctx* ctx, uint32_t n, const float* pos, const float* dir, const float* up, const uint32_t* face_in, const uint32_t* slots,
                       const uint32_t* seed_faces, const float* goal_pos, const float* goal_dir, const mnav_follow_config* config,
                       const mnav_rollout_config* rollout, uint32_t n_candidates, const double* candidates, const mnav_sample_config* sample, uint32_t* best_k_out,
                       double* best_score_out, double* best_cmd_out, uint32_t* n_feasible_out, int32_t* status_out, uint32_t* ticks_out, double* score_out,
                       float* potential_out, uint8_t* lethal_out, double* cost_integral_out, double* travel_out, float* pos_out)
{
  using namespace mnav_smp;
  using mnav_rol::kCounters; using mnav_rol::kStayBlock;
  if (!ctx) return -1;
  ctx->err.clear();
  if (!n) return 0;
  const auto t0 = std::chrono::steady_clock::now();
  // every refusal comes before the first device call: a refused call touches nothing
  std::vector<const float*> maps, pots;
  if (follow_check(ctx, n, pos, dir, up, face_in, slots, seed_faces, config, maps)) return -1;
  if (rollout && rollout->trace_stride) { ctx->err = "sample: trace_stride must be 0 (a sampled rollout leaves no trace)"; return -1; }   // (before the rollout's own trace checks)
  if (rollout_check(ctx, goal_pos, goal_dir, config, rollout, nullptr)) return -1;
  const uint32_t K = n_candidates;
  if (sample_check(ctx, n, slots, config, rollout, K, candidates, sample, pots)) return -1;
  const uint32_t rows = n * K, ticks = rollout->ticks;
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  // the flag is NOT cleared at entry: a control tick cancelled just before its call stays cancelled, and does no work
  if (ctx->cancel.load(std::memory_order_relaxed)) { cancel_reset(ctx); ctx->smp_rec = {}; return 1; }
  if (upload_walk_mesh(ctx)) return -1;
  if (staging_reserve(ctx, rows, ctx->res.plans(), "sample") || rollout_reserve(ctx, "sample", rows, goal_pos != nullptr, ticks, 0) ||
      sample_reserve(ctx, n, rows, K, ctx->res.plans())) return -1;
  mnav_rol::Dev& R = ctx->rol;
  mnav_fol::Staging& G = ctx->stage;
  Dev& D = ctx->smp;
  Stats& rec = ctx->smp_rec;
  rec = {};
  if (locate_ensure(ctx, &rec.rol.built_index)) return -1;            // as the rollouts: the index exists before the first tick
  const mnav_loc::State& L = ctx->loc;
  mnav_rol::Batch B{};
  // the n robots arrive in the front of the staging; all but up (read per robot) move aside before the rows are written over them
  if (staging_upload(ctx, n, pos, dir, up, face_in, slots, seed_faces, maps, B)) return -1;
  HIPCHK(hipMemcpyAsync(D.in_pos, G.pos, 12 * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(D.in_dir, G.dir, 12 * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(D.in_face, G.face, 4 * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(D.in_slot, G.slot, 4 * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
  if (seed_faces) HIPCHK(hipMemcpyAsync(D.in_seed, G.seed_face, 4 * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
  if (goal_pos) {
    HIPCHK(hipMemcpyAsync(R.goal_pos, goal_pos, 12 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(R.goal_dir, goal_dir, 12 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  }
  HIPCHK(hipMemcpyAsync(D.table, candidates, sizeof(Cand) * (size_t)K, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(D.pots, pots.data(), sizeof(const float*) * ctx->res.plans(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(R.cnt, 0, sizeof(uint32_t) * kCounters * (size_t)ticks, ctx->stream));    // every tick's row, once
  HIPCHK(hipMemsetAsync(D.cnt, 0, sizeof(uint32_t) * kPickCounters, ctx->stream));
  B.n = rows;
  B.pos = G.pos; B.dir = G.dir; B.up = G.up; B.face = G.face; B.cnt = R.cnt;
  B.status = R.status; B.ticks = R.ticks; B.travel = R.travel; B.cost_integral = R.cost_integral; B.min_goal_dist = R.min_goal_dist;
  B.goal_pos = goal_pos ? R.goal_pos.get() : nullptr; B.goal_dir = goal_pos ? R.goal_dir.get() : nullptr;
  B.trace = nullptr; B.trace_rows = 0;
  mnav_fol::Config C;
  std::memcpy(&C, config, sizeof(C));
  const Params P{ rollout->dt, (float)rollout->dist_tolerance, (float)rollout->angle_tolerance, goal_pos != nullptr };
  const mnav::WalkMesh M{ ctx->d_xyz, ctx->d_faces, ctx->d_vf_ptr, ctx->d_vf, ctx->V, ctx->F };
  const mnav_loc::Index I{ L.nodes, L.pts, L.n_pts, L.n_leaves, mnav_loc::loc_root(L.n_leaves) };
  Sample X{};
  X.K = K; X.Q = Rule{ C.max_lin_velocity, C.max_ang_velocity, (float)sample->lethal_cost, mnav::GPtr<const uint32_t>(ctx->d_faces), ctx->F };
  X.table = D.table; X.pots = D.pots; X.pot = D.pot; X.lethal = D.lethal; X.cmd0 = D.cmd0;
  const Robots In{ D.in_pos, D.in_dir, D.in_face, D.in_slot, seed_faces ? D.in_seed.get() : nullptr };
  const Weights W{ sample->w_potential, sample->w_cost, sample->w_time, rollout->dt };
  const uint32_t g_rows = (rows + 255u) / 256u, g_stay = (rows + kStayBlock - 1) / kStayBlock, g_search = rows < 2048u ? rows : 2048u;
  const uint32_t g_all = (rows + mnav_loc::kLocBlock - 1) / mnav_loc::kLocBlock, g_global = g_all < 1024u ? g_all : 1024u;
  HIPCHK(hipEventRecord(D.ev[0], ctx->stream));
  hipLaunchKernelGGL(k_sample_expand, dim3(g_rows), dim3(256), 0, ctx->stream, In, B, X, G.slot.get(), G.seed_face.get());
  HIPCHK(hipEventRecord(D.ev[1], ctx->stream));
  float ms_ticks = 0.f;
  // one block: plain launches, no host look in between; then one synchronise
  const auto run_block = [&](uint32_t first, uint32_t nt) -> int {
    HIPCHK(hipEventRecord(G.ev[0], ctx->stream));
    for (uint32_t t = first; t < first + nt; ++t) {
      hipLaunchKernelGGL(k_sample_stay, dim3(g_stay), dim3(kStayBlock), 0, ctx->stream, B, M, C, P, X, t);
      hipLaunchKernelGGL(k_sample_search, dim3(g_search), dim3(64), 0, ctx->stream, B, M, C, P, X, t);
      hipLaunchKernelGGL(k_sample_global, dim3(g_global), dim3(mnav_loc::kLocBlock), 0, ctx->stream, B, M, C, P, X, I, t);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(G.ev[1], ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ms_ticks += ev_ms(G.ev[0], G.ev[1]);
    return 0;
  };
  uint32_t done = 0;
  const int rc = mnav_rol::rol_blocks(ticks, run_block, [&] { return ctx->cancel.load(std::memory_order_relaxed) != 0; }, &done);
  if (rc < 0) return -1;
  rec.ms_expand = ev_ms(D.ev[0], D.ev[1]);
  std::vector<uint32_t> cnt((size_t)kCounters * done);
  uint32_t pick_cnt[kPickCounters] = {};
  HIPCHK(hipMemcpyAsync(cnt.data(), R.cnt, sizeof(uint32_t) * cnt.size(), hipMemcpyDeviceToHost, ctx->stream));
  if (!rc) {                                                          // a cancelled call writes no pick and no row
    HIPCHK(hipEventRecord(D.ev[2], ctx->stream));
    hipLaunchKernelGGL(k_sample_score, dim3(g_rows), dim3(256), 0, ctx->stream, rows, R.status.get(), R.ticks.get(), R.cost_integral.get(), D.pot.get(), D.lethal.get(), W,
                       D.score.get(), D.cnt.get());
    hipLaunchKernelGGL(k_sample_pick, dim3((n + kPickBlock / 64 - 1) / (kPickBlock / 64)), dim3(kPickBlock), 0, ctx->stream, n, K, R.status.get(), D.lethal.get(),
                       D.score.get(), D.cmd0.get(), D.best_k.get(), D.best_score.get(), D.best_cmd.get(), D.n_feasible.get(), D.cnt.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(D.ev[3], ctx->stream));
    HIPCHK(hipMemcpyAsync(pick_cnt, D.cnt, sizeof(pick_cnt), hipMemcpyDeviceToHost, ctx->stream));
    if (best_k_out) HIPCHK(hipMemcpyAsync(best_k_out, D.best_k, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (best_score_out) HIPCHK(hipMemcpyAsync(best_score_out, D.best_score, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (best_cmd_out) HIPCHK(hipMemcpyAsync(best_cmd_out, D.best_cmd, 16 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (n_feasible_out) HIPCHK(hipMemcpyAsync(n_feasible_out, D.n_feasible, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (status_out) HIPCHK(hipMemcpyAsync(status_out, R.status, 4 * (size_t)rows, hipMemcpyDeviceToHost, ctx->stream));
    if (ticks_out) HIPCHK(hipMemcpyAsync(ticks_out, R.ticks, 4 * (size_t)rows, hipMemcpyDeviceToHost, ctx->stream));
    if (score_out) HIPCHK(hipMemcpyAsync(score_out, D.score, 8 * (size_t)rows, hipMemcpyDeviceToHost, ctx->stream));
    if (potential_out) HIPCHK(hipMemcpyAsync(potential_out, D.pot, 4 * (size_t)rows, hipMemcpyDeviceToHost, ctx->stream));
    if (lethal_out) HIPCHK(hipMemcpyAsync(lethal_out, D.lethal, (size_t)rows, hipMemcpyDeviceToHost, ctx->stream));
    if (cost_integral_out) HIPCHK(hipMemcpyAsync(cost_integral_out, R.cost_integral, 8 * (size_t)rows, hipMemcpyDeviceToHost, ctx->stream));
    if (travel_out) HIPCHK(hipMemcpyAsync(travel_out, R.travel, 8 * (size_t)rows, hipMemcpyDeviceToHost, ctx->stream));
    if (pos_out) HIPCHK(hipMemcpyAsync(pos_out, G.pos, 12 * (size_t)rows, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (!rc) rec.ms_pick = ev_ms(D.ev[2], D.ev[3]);
  else cancel_reset(ctx);                                             // the call that honoured the flag takes it down
  mnav_rol::rol_fold_counters(cnt.data(), done, rows, rec.rol);
  rec.lethal_rows = pick_cnt[kCntLethal]; rec.feasible_rows = pick_cnt[kCntFeasible]; rec.robots_without_pick = pick_cnt[kCntNoPick];
  rec.rol.ms_kernels = rec.ms_expand + ms_ticks + rec.ms_pick;
  rec.rol.ms_total = (float)(1e-3 * (double)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count());
  return rc;
}

int mnav_sample_stats(const mnav_ctx* ctx, uint32_t* status_counts, uint32_t* lethal_rows, uint32_t* feasible_rows, uint32_t* robots_without_pick, uint64_t* row_ticks,
                      uint64_t* stayed, uint64_t* neighbour, uint64_t* global, uint32_t* built_index, float* ms_expand, float* ms_pick, float* ms_kernels, float* ms_total)
{
  if (!ctx) return -1;
  const mnav_smp::Stats& S = ctx->smp_rec;
  rollout_stats_get(S.rol, status_counts, row_ticks, stayed, neighbour, global, built_index, ms_kernels, ms_total);
  if (lethal_rows) *lethal_rows = S.lethal_rows;
  if (feasible_rows) *feasible_rows = S.feasible_rows;
  if (robots_without_pick) *robots_without_pick = S.robots_without_pick;
  if (ms_expand) *ms_expand = S.ms_expand;
  if (ms_pick) *ms_pick = S.ms_pick;
  return 0;
}
