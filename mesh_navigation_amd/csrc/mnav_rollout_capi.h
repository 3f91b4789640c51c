// mnav_rollout_capi.h -- the C ABI of the device rollouts (include/mnav.h: mnav_follow_rollout, mnav_rollout_stats,
// mnav_fleet_rollout, mnav_fleet_rollout_stats, mnav_fleet_rollout_yield, mnav_fleet_yield_stats, mnav_fleet_rollout_rings,
// mnav_fleet_ring_stats) over the kernels of mnav_rollout.h, mnav_fleet_rollout.h, mnav_fleet_yield.h and mnav_fleet_ring.h.  Included by
// mnav.hip inside its extern "C" block, after mnav_follow_capi.h (the argument checks are the follower's) and
// mnav_locate_capi.h (the index build is the lookup's own).  One driver, rollout_run, holds the call; the four entry points
// hand it one RolloutCall with their arguments and their own statistics record.  The device buffers are shared (a call uploads every input at
// entry), the statistics are kept apart: a call of one entry point leaves what the other's *_stats tells alone.
#pragma once

static_assert(mnav_frol::kWaitingPresent == MNAV_SEP_WAITING_PRESENT && mnav_frol::kReachedPresent == MNAV_SEP_REACHED_PRESENT,
              "mnav_fleet_rollout.h restates the values of include/mnav.h");
static_assert(mnav_frol::kRingRelease == MNAV_RING_RELEASE && mnav_frol::kWaitFree == MNAV_WAIT_FREE && mnav_frol::kWaitQueued == MNAV_WAIT_QUEUED &&
              mnav_frol::kWaitParked == MNAV_WAIT_PARKED && mnav_frol::kWaitRingTail == MNAV_WAIT_RING_TAIL && mnav_frol::kWaitRingMember == MNAV_WAIT_RING_MEMBER,
              "mnav_fleet_ring.h restates the values of include/mnav.h");

// (the counter rows' message names the entry point, the others the rollout, as callers have seen them)
static int rollout_reserve(mnav_ctx* ctx, const char* tag, size_t n, bool goals, size_t ticks, size_t trace_floats)
{
  mnav_rol::Dev& S = ctx->rol;
  const char* oom = "rollout: out of device memory";
  if (n > S.cap) {
    S.cap = 0;
    if (alloc_group(S.status, 4 * n, S.ticks, 4 * n, S.travel, 8 * n, S.cost_integral, 8 * n, S.min_goal_dist, 4 * n) != hipSuccess) { ctx->err = oom; return -1; }
    S.goal_pos.reset(); S.goal_dir.reset();
    S.cap = n;
  }
  if (goals && !S.goal_pos && alloc_group(S.goal_pos, 12 * S.cap, S.goal_dir, 12 * S.cap) != hipSuccess) { ctx->err = oom; return -1; }
  if (ticks > S.cnt_cap) {
    S.cnt_cap = 0;
    if (S.cnt.alloc(sizeof(uint32_t) * mnav_rol::kCounters * ticks) != hipSuccess) { ctx->err = std::string(tag) + ": out of device memory"; return -1; }
    S.cnt_cap = ticks;
  }
  if (trace_floats > S.trace_cap) {
    S.trace_cap = 0;
    if (S.trace.alloc(sizeof(float) * trace_floats) != hipSuccess) { ctx->err = oom; return -1; }
    S.trace_cap = trace_floats;
  }
  return 0;
}

// what start ticks and a separation check need beside the rollout's buffers
static int fleet_rollout_reserve(mnav_ctx* ctx, size_t n, bool starts, bool sep, size_t table, size_t checks)
{
  mnav_frol::State& S = ctx->frol;
  const char* oom = "fleet rollout: out of device memory";
  if (starts && n > S.cap) {
    S.cap = 0;
    if (S.start_tick.alloc(4 * n) != hipSuccess) { ctx->err = oom; return -1; }
    S.cap = n;
  }
  if (!sep) return 0;
  if (!S.have_ev) {                                                   // only a check records them: a call without one creates none
    for (auto& e : S.ev) HIPCHK(hipEventCreate(e.out()));
    S.have_ev = true;
  }
  if (n > S.sep_cap) {
    S.sep_cap = 0;
    if (alloc_group(S.slot_of, 4 * n, S.rank, 4 * n, S.rec, 16 * n, S.near_checks, 4 * n, S.max_partners, 4 * n, S.first_near_tick, 4 * n, S.first_near_robot, 4 * n,
                    S.min_sep2, 4 * n, S.min_sep_tick, 4 * n, S.min_sep_robot, 4 * n) != hipSuccess) { ctx->err = oom; return -1; }
    S.sep_cap = n;
  }
  if (table > S.table_cap) {
    S.table_cap = 0;
    if (alloc_group(S.keys, 8 * table, S.cell_cnt, 4 * table, S.cell_start, 4 * table, S.tile, 4 * ((table + mnav_frol::kSepTile - 1) / mnav_frol::kSepTile)) != hipSuccess) {
      ctx->err = oom; return -1;
    }
    S.table_cap = table;
  }
  if (checks > S.chk_cap) {
    S.chk_cap = 0;
    if (S.chk.alloc(sizeof(unsigned long long) * mnav_frol::kCheckWords * checks) != hipSuccess) { ctx->err = oom; return -1; }
    S.chk_cap = checks;
  }
  return 0;
}

// what the right-of-way rule needs beside the separation check's buffers
static int fleet_yield_reserve(mnav_ctx* ctx, size_t n, size_t checks)
{
  mnav_frol::YldState& Y = ctx->yld;
  const char* oom = "fleet rollout yield: out of device memory";
  if (!Y.have_ev) {
    for (auto& e : Y.ev) HIPCHK(hipEventCreate(e.out()));
    Y.have_ev = true;
  }
  if (n > Y.cap) {
    Y.cap = 0;
    if (alloc_group(Y.hold, n, Y.priority, 4 * n, Y.hold_checks, 4 * n, Y.held_ticks, 4 * n, Y.first_hold_tick, 4 * n, Y.first_hold_robot, 4 * n) != hipSuccess) {
      ctx->err = oom; return -1;
    }
    Y.cap = n;
  }
  if (checks > Y.chk_cap) {
    Y.chk_cap = 0;
    if (Y.ychk.alloc(sizeof(uint32_t) * mnav_frol::kYldCheckWords * checks) != hipSuccess) { ctx->err = oom; return -1; }
    Y.chk_cap = checks;
  }
  return 0;
}

// what the wait-for analysis needs beside the rule's buffers
static int fleet_ring_reserve(mnav_ctx* ctx, size_t n, size_t checks)
{
  mnav_frol::RingState& W = ctx->ring;
  const char* oom = "fleet rollout rings: out of device memory";
  if (!W.have_ev) {
    for (auto& e : W.ev) HIPCHK(hipEventCreate(e.out()));
    W.have_ev = true;
  }
  if (n > W.cap) {
    W.cap = 0;
    if (alloc_group(W.blocker, 4 * n, W.jump0, 4 * n, W.jump1, 4 * n, W.key0, 8 * n, W.key1, 8 * n, W.mark, n, W.wait_class, n, W.anchor, 4 * n, W.ring_checks, 4 * n,
                    W.first_ring_tick, 4 * n, W.parked_checks, 4 * n, W.released_checks, 4 * n) != hipSuccess) {
      ctx->err = oom; return -1;
    }
    W.cap = n;
  }
  if (checks > W.chk_cap) {
    W.chk_cap = 0;
    if (W.rchk.alloc(sizeof(uint32_t) * mnav_frol::kRingCheckWords * checks) != hipSuccess) { ctx->err = oom; return -1; }
    W.chk_cap = checks;
  }
  return 0;
}

// The optional last input of rollout_run: the right-of-way rule of mnav_fleet_rollout_yield.  config null: no rule, and then
// every other pointer must be null; host pointers, each output may be null.
struct YieldCall {
  const mnav_yield_config* config = nullptr; const uint32_t* priority = nullptr; const uint8_t* hold_in = nullptr; uint8_t* hold_out = nullptr;
  mnav_frol::YRows out = { nullptr, nullptr, nullptr, nullptr };
};

// ... and behind it the wait-for analysis of mnav_fleet_rollout_rings.  config null: no analysis, and then every output must be
// null; host pointers, each output may be null.
struct RingCall {
  const mnav_ring_config* config = nullptr;
  mnav_frol::RRows out = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
};

// One call of rollout_run, as its entry point fills it.  tag names the entry point in the messages that do, rec is the record
// its *_stats functions read.  start_tick: null, or a departure tick per robot; separation: null, or the check, whose
// per-robot outputs go to sep_out; yld: the rule inside the check, or one without a config.  Host pointers; each output may be
// null, and all of sep_out are without a separation.
struct RolloutCall {
  const char* tag; mnav_ctx::RolloutRecord* rec;
  uint32_t n; const float* pos; const float* dir; const float* up; const uint32_t* face_in; const uint32_t* slots; const uint32_t* seed_faces;
  const float* goal_pos; const float* goal_dir; const mnav_follow_config* config; const mnav_rollout_config* rollout;
  const uint32_t* start_tick; const mnav_separation_config* separation;
  struct { int32_t* status; uint32_t* ticks; float* pos; float* dir; uint32_t* face; double* travel; double* cost_integral; float* min_goal_dist; float* trace; } out;
  mnav_frol::Rows sep_out; YieldCall yld; RingCall ring;
};

// The argument checks of a rollout beside the follower's, all on the host: -1 with ctx->err set, or 0.
static int rollout_check(mnav_ctx* ctx, const float* goal_pos, const float* goal_dir, const mnav_follow_config* config, const mnav_rollout_config* rollout,
                         const float* trace_out)
{
  using namespace mnav_rol;
  if (!rollout) { ctx->err = "rollout: null argument"; return -1; }
  if (!(rollout->dt > 0.0) || !std::isfinite(rollout->dt)) { ctx->err = "rollout: dt must be positive and finite"; return -1; }
  if (rollout->ticks < 1 || rollout->ticks > kMaxTicks) { ctx->err = "rollout: ticks out of range (1 .. 100000)"; return -1; }
  if (rollout->trace_stride && !trace_out) { ctx->err = "rollout: trace_stride without trace_out"; return -1; }
  if (rollout->trace_stride > rollout->ticks) { ctx->err = "rollout: trace_stride larger than ticks"; return -1; }
  if (!goal_pos != !goal_dir) { ctx->err = "rollout: goal_pos and goal_dir go together"; return -1; }
  if (std::isnan(rollout->dist_tolerance) || std::isnan(rollout->angle_tolerance)) { ctx->err = "rollout: dist_tolerance / angle_tolerance is NaN"; return -1; }
  // the restated sinf / cosf are the host libm's on (-120, 120) only; NaN parameters give NaN commands, which std::min caps
  const double turn = std::fabs(config->max_ang_velocity) * std::fmax(1.0, std::fabs(config->ang_vel_factor)) * rollout->dt;   // bounds |ang * dt|
  if (!(turn < 100.0)) { ctx->err = "rollout: max_ang_velocity * max(1, ang_vel_factor) * dt must stay below 100 rad per tick"; return -1; }
  return 0;
}

// The whole call of every entry point.  Returns 0, 1 when cancelled, 2 when a check was skipped, -1 with ctx->err set.
static int rollout_run(mnav_ctx* ctx, const RolloutCall& A)
{
  using namespace mnav_frol;
  using mnav_rol::Batch; using mnav_rol::kCounters; using mnav_rol::kStayBlock; using mnav_rol::Params; using mnav::WalkMesh;
  const uint32_t n = A.n;
  ctx->err.clear();
  if (!n) return 0;
  const auto t0 = std::chrono::steady_clock::now();
  // every refusal comes before the first device call: a refused call touches nothing
  std::vector<const float*> maps;
  if (follow_check(ctx, n, A.pos, A.dir, A.up, A.face_in, A.slots, A.seed_faces, A.config, maps)) return -1;
  if (rollout_check(ctx, A.goal_pos, A.goal_dir, A.config, A.rollout, A.out.trace)) return -1;
  const uint32_t ticks = A.rollout->ticks, stride = A.rollout->trace_stride, rows = stride ? ticks / stride : 0;
  Grid grid{};
  uint32_t check_stride = 0, flags = 0;
  if (!A.separation) {
    if (A.sep_out.near_checks || A.sep_out.max_partners || A.sep_out.first_near_tick || A.sep_out.first_near_robot || A.sep_out.min_sep2 || A.sep_out.min_sep_tick ||
        A.sep_out.min_sep_robot) {
      ctx->err = "fleet rollout: a separation output without a separation config"; return -1;
    }
  } else {
    double scale = opt_set(ctx->opt.separation_cell_scale) ? ctx->opt.separation_cell_scale : (double)kDefaultCellScale;
    if (!(scale >= 1.0 && scale <= 4.0)) { ctx->err = "fleet rollout: separation_cell_scale outside 1 .. 4"; return -1; }
    grid = sep_grid((float)A.separation->radius, (float)scale);
    if (!((float)A.separation->radius > 0.f) || !sep_grid_ok(grid)) { ctx->err = "fleet rollout: radius: (float)radius must be positive, its square finite and positive"; return -1; }
    check_stride = A.separation->check_stride; flags = A.separation->flags;
    if (check_stride < 1 || check_stride > ticks) { ctx->err = "fleet rollout: check_stride outside 1 .. ticks"; return -1; }
    if (flags & ~kKnownFlags) { ctx->err = "fleet rollout: unknown separation flag"; return -1; }
  }
  const bool yielding = A.yld.config != nullptr;
  float ahead_c2 = 0.f;
  if (!yielding) {
    if (A.yld.priority || A.yld.hold_in || A.yld.hold_out || A.yld.out.hold_checks || A.yld.out.held_ticks || A.yld.out.first_hold_tick || A.yld.out.first_hold_robot) {
      ctx->err = "fleet rollout yield: a yield input or output without a yield config"; return -1;
    }
  } else {
    if (!A.separation) { ctx->err = "fleet rollout yield: a yield config without a separation config"; return -1; }
    const float c = (float)A.yld.config->ahead_cos;
    if (!yld_cos_ok(c)) { ctx->err = "fleet rollout yield: ahead_cos: (float)ahead_cos must be finite, at least 0 and below 1"; return -1; }
    if (A.yld.config->flags) { ctx->err = "fleet rollout yield: the flags of the yield config are reserved and must be 0"; return -1; }
    ahead_c2 = c * c;
  }
  const bool rings = A.ring.config != nullptr;
  if (!rings) {
    if (A.ring.out.ring_checks || A.ring.out.first_ring_tick || A.ring.out.parked_checks || A.ring.out.released_checks || A.ring.out.wait_class || A.ring.out.anchor) {
      ctx->err = "fleet rollout rings: a ring output without a ring config"; return -1;
    }
  } else {
    if (!yielding) { ctx->err = "fleet rollout rings: a ring config without a yield config"; return -1; }
    if (A.ring.config->flags & ~kRingKnownFlags) { ctx->err = "fleet rollout rings: unknown ring flag"; return -1; }
  }
  const uint32_t checks = A.separation ? ticks / check_stride : 0, table = A.separation ? sep_table_size(n) : 0;
  const double max_tests_d = opt_set(ctx->opt.separation_max_tests) ? std::max(ctx->opt.separation_max_tests, 0.0) : kDefaultMaxTests;
  const unsigned long long max_tests = max_tests_d >= 18446744073709551615.0 ? ~0ull : (unsigned long long)max_tests_d;
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  cancel_reset(ctx);                                                  // as the plan calls do
  if (upload_walk_mesh(ctx)) return -1;
  if (staging_reserve(ctx, n, ctx->res.plans(), A.tag) || rollout_reserve(ctx, A.tag, n, A.goal_pos != nullptr, ticks, 3 * (size_t)n * rows) ||
      fleet_rollout_reserve(ctx, n, A.start_tick != nullptr || yielding, A.separation != nullptr, table, checks) || (yielding && fleet_yield_reserve(ctx, n, checks)) ||
      (rings && fleet_ring_reserve(ctx, n, checks))) return -1;
  mnav_rol::Dev& R = ctx->rol;
  State& S = ctx->frol;
  YldState& Y = ctx->yld;
  RingState& W = ctx->ring;
  mnav_fol::Staging& G = ctx->stage;
  mnav_ctx::RolloutRecord& rec = *A.rec;
  rec = {};
  if (locate_ensure(ctx, &rec.rol.built_index)) return -1;            // no look at the lists between ticks: the index exists before the first one
  const mnav_loc::State& L = ctx->loc;
  Batch B{};
  if (staging_upload(ctx, n, A.pos, A.dir, A.up, A.face_in, A.slots, A.seed_faces, maps, B)) return -1;
  if (A.goal_pos) {
    HIPCHK(hipMemcpyAsync(R.goal_pos, A.goal_pos, 12 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(R.goal_dir, A.goal_dir, 12 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  }
  if (A.start_tick) HIPCHK(hipMemcpyAsync(S.start_tick, A.start_tick, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  else if (yielding) HIPCHK(hipMemsetAsync(S.start_tick, 0, 4 * (size_t)n, ctx->stream));   // FleetTick's start ticks are never null
  std::vector<uint8_t> h_hold;                                        // hold_in as flags; lives until the synchronise of the first block
  HIPCHK(hipMemsetAsync(R.status, 0, 4 * (size_t)n, ctx->stream));    // kRunning
  HIPCHK(hipMemsetAsync(R.ticks, 0, 4 * (size_t)n, ctx->stream));
  HIPCHK(hipMemsetAsync(R.travel, 0, 8 * (size_t)n, ctx->stream));
  HIPCHK(hipMemsetAsync(R.cost_integral, 0, 8 * (size_t)n, ctx->stream));
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)R.min_goal_dist.get(), 0x7F800000, n, ctx->stream));   // +inf
  HIPCHK(hipMemsetAsync(R.cnt, 0, sizeof(uint32_t) * kCounters * (size_t)ticks, ctx->stream));    // every tick's row, once
  B.pos = G.pos; B.dir = G.dir; B.up = G.up; B.face = G.face; B.cnt = R.cnt;
  B.status = R.status; B.ticks = R.ticks; B.travel = R.travel; B.cost_integral = R.cost_integral; B.min_goal_dist = R.min_goal_dist;
  B.goal_pos = A.goal_pos ? R.goal_pos.get() : nullptr; B.goal_dir = A.goal_pos ? R.goal_dir.get() : nullptr;
  B.trace = rows ? R.trace.get() : nullptr; B.trace_rows = rows;
  const uint32_t* d_start = A.start_tick || yielding ? S.start_tick.get() : nullptr;
  Sep Q{};
  Yld YQ{};
  Ring WQ{};
  if (A.separation) {
    HIPCHK(hipMemsetAsync(S.near_checks, 0, 4 * (size_t)n, ctx->stream));                          // sep_row_start
    HIPCHK(hipMemsetAsync(S.max_partners, 0, 4 * (size_t)n, ctx->stream));
    HIPCHK(hipMemsetAsync(S.first_near_tick, 0xFF, 4 * (size_t)n, ctx->stream));
    HIPCHK(hipMemsetAsync(S.first_near_robot, 0xFF, 4 * (size_t)n, ctx->stream));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)S.min_sep2.get(), 0x7F800000, n, ctx->stream));
    HIPCHK(hipMemsetAsync(S.min_sep_tick, 0xFF, 4 * (size_t)n, ctx->stream));
    HIPCHK(hipMemsetAsync(S.min_sep_robot, 0xFF, 4 * (size_t)n, ctx->stream));
    HIPCHK(hipMemsetAsync(S.chk, 0, sizeof(unsigned long long) * kCheckWords * (size_t)checks, ctx->stream));
    Q.n = n; Q.flags = flags; Q.mask = table - 1; Q.tiles = (table + kSepTile - 1) / kSepTile; Q.G = grid; Q.max_tests = max_tests;
    Q.pos = G.pos; Q.status = R.status; Q.start_tick = d_start;
    Q.keys = S.keys; Q.cnt = S.cell_cnt; Q.start = S.cell_start; Q.tile = S.tile; Q.slot_of = S.slot_of; Q.rank = S.rank; Q.rec = S.rec; Q.chk = S.chk;
    Q.rows = Rows{ S.near_checks, S.max_partners, S.first_near_tick, S.first_near_robot, S.min_sep2, S.min_sep_tick, S.min_sep_robot };
  }
  if (yielding) {
    if (A.yld.hold_in) {                                              // any non-zero byte is 1
      h_hold.assign(A.yld.hold_in, A.yld.hold_in + n);
      for (auto& b : h_hold) b = b != 0;
      HIPCHK(hipMemcpyAsync(Y.hold, h_hold.data(), n, hipMemcpyHostToDevice, ctx->stream));
    } else HIPCHK(hipMemsetAsync(Y.hold, 0, n, ctx->stream));
    if (A.yld.priority) HIPCHK(hipMemcpyAsync(Y.priority, A.yld.priority, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(Y.hold_checks, 0, 4 * (size_t)n, ctx->stream));                           // yld_row_start
    HIPCHK(hipMemsetAsync(Y.held_ticks, 0, 4 * (size_t)n, ctx->stream));
    HIPCHK(hipMemsetAsync(Y.first_hold_tick, 0xFF, 4 * (size_t)n, ctx->stream));
    HIPCHK(hipMemsetAsync(Y.first_hold_robot, 0xFF, 4 * (size_t)n, ctx->stream));
    HIPCHK(hipMemsetAsync(Y.ychk, 0, sizeof(uint32_t) * kYldCheckWords * (size_t)checks, ctx->stream));
    YQ.c2 = ahead_c2; YQ.dir = G.dir; YQ.priority = A.yld.priority ? Y.priority.get() : nullptr; YQ.hold = Y.hold; YQ.ychk = Y.ychk;
    YQ.rows = YRows{ Y.hold_checks, Y.held_ticks, Y.first_hold_tick, Y.first_hold_robot };
  }
  if (rings) {
    HIPCHK(hipMemsetAsync(W.wait_class, 0, n, ctx->stream));                                        // kWaitFree: no check ran yet
    HIPCHK(hipMemsetAsync(W.anchor, 0xFF, 4 * (size_t)n, ctx->stream));
    HIPCHK(hipMemsetAsync(W.ring_checks, 0, 4 * (size_t)n, ctx->stream));
    HIPCHK(hipMemsetAsync(W.first_ring_tick, 0xFF, 4 * (size_t)n, ctx->stream));
    HIPCHK(hipMemsetAsync(W.parked_checks, 0, 4 * (size_t)n, ctx->stream));
    HIPCHK(hipMemsetAsync(W.released_checks, 0, 4 * (size_t)n, ctx->stream));
    HIPCHK(hipMemsetAsync(W.rchk, 0, sizeof(uint32_t) * kRingCheckWords * (size_t)checks, ctx->stream));
    WQ.flags = A.ring.config->flags; WQ.early = opt_on(ctx->opt.ring_early_exit); WQ.launched = ring_launches(n);
    WQ.blocker = W.blocker; WQ.jump[0] = W.jump0; WQ.jump[1] = W.jump1; WQ.key[0] = W.key0; WQ.key[1] = W.key1; WQ.mark = W.mark; WQ.rchk = W.rchk;
    WQ.rows = RRows{ W.ring_checks, W.first_ring_tick, W.parked_checks, W.released_checks, W.wait_class, W.anchor };
  }
  mnav_fol::Config C;
  std::memcpy(&C, A.config, sizeof(C));
  const Params P{ A.rollout->dt, (float)A.rollout->dist_tolerance, (float)A.rollout->angle_tolerance, A.goal_pos != nullptr };
  const WalkMesh M{ ctx->d_xyz, ctx->d_faces, ctx->d_vf_ptr, ctx->d_vf, ctx->V, ctx->F };
  const mnav_loc::Index I{ L.nodes, L.pts, L.n_pts, L.n_leaves, mnav_loc::loc_root(L.n_leaves) };
  const uint32_t g_stay = (n + kStayBlock - 1) / kStayBlock, g_search = n < 2048u ? n : 2048u;
  const uint32_t g_all = (n + mnav_loc::kLocBlock - 1) / mnav_loc::kLocBlock, g_global = g_all < 1024u ? g_all : 1024u;
  const uint32_t g_sep = (n + kSepBlock - 1) / kSepBlock, g_clear = Q.tiles < 4096u ? Q.tiles : 4096u;
  float ms_kernels = 0.f, ms_separation = 0.f, ms_pair = 0.f, ms_ring = 0.f;
  // one block: plain launches, no host look in between; then one synchronise
  const auto run_block = [&](uint32_t first, uint32_t nt) -> int {
    HIPCHK(hipEventRecord(G.ev[0], ctx->stream));
    uint32_t in_block = 0;
    for (uint32_t t = first; t < first + nt; ++t) {
      const uint32_t row = stride && (t + 1) % stride == 0 ? (t + 1) / stride - 1 : kNone;
      if (yielding) {                                                 // a held robot has no tick
        hipLaunchKernelGGL(k_yield_rollout_stay, dim3(g_stay), dim3(kStayBlock), 0, ctx->stream, B, M, C, P, t, row, d_start, YQ.hold, YQ.rows.held_ticks);
        hipLaunchKernelGGL(k_yield_rollout_search, dim3(g_search), dim3(64), 0, ctx->stream, B, M, C, P, t, row, d_start, YQ.hold, YQ.rows.held_ticks);
        hipLaunchKernelGGL(k_yield_rollout_global, dim3(g_global), dim3(mnav_loc::kLocBlock), 0, ctx->stream, B, M, C, P, I, t, row, d_start, YQ.hold, YQ.rows.held_ticks);
      } else if (d_start) {
        hipLaunchKernelGGL(k_fleet_rollout_stay, dim3(g_stay), dim3(kStayBlock), 0, ctx->stream, B, M, C, P, t, row, d_start);
        hipLaunchKernelGGL(k_fleet_rollout_search, dim3(g_search), dim3(64), 0, ctx->stream, B, M, C, P, t, row, d_start);
        hipLaunchKernelGGL(k_fleet_rollout_global, dim3(g_global), dim3(mnav_loc::kLocBlock), 0, ctx->stream, B, M, C, P, I, t, row, d_start);
      } else {                                                        // nobody waits: the rollout's own passes, the same bits
        hipLaunchKernelGGL(mnav_rol::k_rollout_stay, dim3(g_stay), dim3(kStayBlock), 0, ctx->stream, B, M, C, P, t, row);
        hipLaunchKernelGGL(mnav_rol::k_rollout_search, dim3(g_search), dim3(64), 0, ctx->stream, B, M, C, P, t, row);
        hipLaunchKernelGGL(mnav_rol::k_rollout_global, dim3(g_global), dim3(mnav_loc::kLocBlock), 0, ctx->stream, B, M, C, P, I, t, row);
      }
      if (!A.separation || (t + 1) % check_stride) continue;
      const uint32_t check = (t + 1) / check_stride - 1;
      HIPCHK(hipEventRecord(S.ev[2 * in_block], ctx->stream));
      hipLaunchKernelGGL(k_sep_clear, dim3(g_clear), dim3(kSepBlock), 0, ctx->stream, Q);
      hipLaunchKernelGGL(k_sep_insert, dim3(g_sep), dim3(kSepBlock), 0, ctx->stream, Q, t + 1);
      hipLaunchKernelGGL(k_sep_sums, dim3(Q.tiles), dim3(kSepBlock), 0, ctx->stream, Q);
      hipLaunchKernelGGL(k_sep_top, dim3(1), dim3(kSepBlock), 0, ctx->stream, Q);
      hipLaunchKernelGGL(k_sep_starts, dim3(Q.tiles), dim3(kSepBlock), 0, ctx->stream, Q);
      hipLaunchKernelGGL(k_sep_fill, dim3(g_sep), dim3(kSepBlock), 0, ctx->stream, Q, check);
      if (rings) {                                                    // the pair pass that keeps the blockers, then the analysis
        HIPCHK(hipEventRecord(Y.ev[2 * in_block], ctx->stream));
        hipLaunchKernelGGL(k_ring_pair, dim3(g_sep), dim3(kSepBlock), 0, ctx->stream, Q, YQ, WQ, check, t + 1);
        HIPCHK(hipEventRecord(Y.ev[2 * in_block + 1], ctx->stream));
        HIPCHK(hipEventRecord(W.ev[2 * in_block], ctx->stream));
        for (uint32_t k = 0; k < WQ.launched; ++k) hipLaunchKernelGGL(k_ring_double, dim3(g_sep), dim3(kSepBlock), 0, ctx->stream, WQ, n, YQ.ychk, check, k);
        hipLaunchKernelGGL(k_ring_close, dim3(g_sep), dim3(kSepBlock), 0, ctx->stream, Q, WQ, YQ.ychk, check, t + 1);
        hipLaunchKernelGGL(k_ring_rows, dim3(g_sep), dim3(kSepBlock), 0, ctx->stream, WQ, n, YQ.hold, check, t + 1);
        HIPCHK(hipEventRecord(W.ev[2 * in_block + 1], ctx->stream));
      } else if (yielding) {
        HIPCHK(hipEventRecord(Y.ev[2 * in_block], ctx->stream));
        hipLaunchKernelGGL(k_yld_pair, dim3(g_sep), dim3(kSepBlock), 0, ctx->stream, Q, YQ, check, t + 1);
        HIPCHK(hipEventRecord(Y.ev[2 * in_block + 1], ctx->stream));
      } else hipLaunchKernelGGL(k_sep_pair, dim3(g_sep), dim3(kSepBlock), 0, ctx->stream, Q, check, t + 1);
      HIPCHK(hipEventRecord(S.ev[2 * in_block + 1], ctx->stream));
      ++in_block;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(G.ev[1], ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ms_kernels += ev_ms(G.ev[0], G.ev[1]);
    for (uint32_t k = 0; k < in_block; ++k) ms_separation += ev_ms(S.ev[2 * k], S.ev[2 * k + 1]);
    if (yielding) for (uint32_t k = 0; k < in_block; ++k) ms_pair += ev_ms(Y.ev[2 * k], Y.ev[2 * k + 1]);
    if (rings) for (uint32_t k = 0; k < in_block; ++k) ms_ring += ev_ms(W.ev[2 * k], W.ev[2 * k + 1]);
    return 0;
  };
  uint32_t done = 0;
  const int rc = mnav_rol::rol_blocks(ticks, run_block, [&] { return ctx->cancel.load(std::memory_order_relaxed) != 0; }, &done);
  if (rc < 0) return -1;
  const uint32_t checks_done = A.separation ? done / check_stride : 0;
  std::vector<uint32_t> cnt((size_t)kCounters * done);
  std::vector<uint64_t> chk((size_t)kCheckWords * checks_done);
  std::vector<uint32_t> h_near, h_robot; std::vector<float> h_min;
  std::vector<uint32_t> ychk((size_t)kYldCheckWords * (yielding ? checks_done : 0)), h_hold_checks, h_held_ticks;
  HIPCHK(hipMemcpyAsync(cnt.data(), R.cnt, sizeof(uint32_t) * cnt.size(), hipMemcpyDeviceToHost, ctx->stream));
  if (A.out.status) HIPCHK(hipMemcpyAsync(A.out.status, R.status, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (A.out.ticks) HIPCHK(hipMemcpyAsync(A.out.ticks, R.ticks, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (A.out.pos) HIPCHK(hipMemcpyAsync(A.out.pos, G.pos, 12 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (A.out.dir) HIPCHK(hipMemcpyAsync(A.out.dir, G.dir, 12 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (A.out.face) HIPCHK(hipMemcpyAsync(A.out.face, G.face, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (A.out.travel) HIPCHK(hipMemcpyAsync(A.out.travel, R.travel, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (A.out.cost_integral) HIPCHK(hipMemcpyAsync(A.out.cost_integral, R.cost_integral, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (A.out.min_goal_dist) HIPCHK(hipMemcpyAsync(A.out.min_goal_dist, R.min_goal_dist, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (rows) HIPCHK(hipMemcpyAsync(A.out.trace, R.trace, 12 * (size_t)n * rows, hipMemcpyDeviceToHost, ctx->stream));   // (rows past a cancel are not written)
  if (A.separation) {
    h_near.resize(n); h_robot.resize(n); h_min.resize(n);             // the statistics read three of the rows' columns
    if (checks_done) HIPCHK(hipMemcpyAsync(chk.data(), S.chk, sizeof(uint64_t) * chk.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h_near.data(), S.near_checks, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h_min.data(), S.min_sep2, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h_robot.data(), S.min_sep_robot, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (A.sep_out.max_partners) HIPCHK(hipMemcpyAsync(A.sep_out.max_partners, S.max_partners, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (A.sep_out.first_near_tick) HIPCHK(hipMemcpyAsync(A.sep_out.first_near_tick, S.first_near_tick, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (A.sep_out.first_near_robot) HIPCHK(hipMemcpyAsync(A.sep_out.first_near_robot, S.first_near_robot, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (A.sep_out.min_sep_tick) HIPCHK(hipMemcpyAsync(A.sep_out.min_sep_tick, S.min_sep_tick, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (yielding) {
    h_hold_checks.resize(n); h_held_ticks.resize(n); h_hold.resize(n); // the statistics read two of the yield rows' columns and the flags
    if (checks_done) HIPCHK(hipMemcpyAsync(ychk.data(), Y.ychk, sizeof(uint32_t) * ychk.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h_hold_checks.data(), Y.hold_checks, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h_held_ticks.data(), Y.held_ticks, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h_hold.data(), Y.hold, n, hipMemcpyDeviceToHost, ctx->stream));
    if (A.yld.out.first_hold_tick) HIPCHK(hipMemcpyAsync(A.yld.out.first_hold_tick, Y.first_hold_tick, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (A.yld.out.first_hold_robot) HIPCHK(hipMemcpyAsync(A.yld.out.first_hold_robot, Y.first_hold_robot, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  }
  std::vector<uint32_t> rchk((size_t)kRingCheckWords * (rings ? checks_done : 0)), h_ring_checks;
  if (rings) {
    h_ring_checks.resize(n);                                          // the statistics read one of the ring rows' columns
    if (checks_done) HIPCHK(hipMemcpyAsync(rchk.data(), W.rchk, sizeof(uint32_t) * rchk.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h_ring_checks.data(), W.ring_checks, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (A.ring.out.first_ring_tick) HIPCHK(hipMemcpyAsync(A.ring.out.first_ring_tick, W.first_ring_tick, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (A.ring.out.parked_checks) HIPCHK(hipMemcpyAsync(A.ring.out.parked_checks, W.parked_checks, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (A.ring.out.released_checks) HIPCHK(hipMemcpyAsync(A.ring.out.released_checks, W.released_checks, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (A.ring.out.wait_class) HIPCHK(hipMemcpyAsync(A.ring.out.wait_class, W.wait_class, n, hipMemcpyDeviceToHost, ctx->stream));
    if (A.ring.out.anchor) HIPCHK(hipMemcpyAsync(A.ring.out.anchor, W.anchor, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  mnav_rol::rol_fold_counters(cnt.data(), done, n, rec.rol);
  if (A.separation) {
    sep_fold(chk.data(), checks_done, check_stride, n, h_near.data(), h_min.data(), h_robot.data(), rec.sep);
    if (A.sep_out.near_checks) std::memcpy(A.sep_out.near_checks, h_near.data(), 4 * (size_t)n);
    if (A.sep_out.min_sep2) std::memcpy(A.sep_out.min_sep2, h_min.data(), 4 * (size_t)n);
    if (A.sep_out.min_sep_robot) std::memcpy(A.sep_out.min_sep_robot, h_robot.data(), 4 * (size_t)n);
  }
  if (yielding) {
    yld_fold(chk.data(), ychk.data(), checks_done, check_stride, n, h_hold_checks.data(), h_held_ticks.data(), h_hold.data(), rec.yld);
    if (A.yld.out.hold_checks) std::memcpy(A.yld.out.hold_checks, h_hold_checks.data(), 4 * (size_t)n);
    if (A.yld.out.held_ticks) std::memcpy(A.yld.out.held_ticks, h_held_ticks.data(), 4 * (size_t)n);
    if (A.yld.hold_out) std::memcpy(A.yld.hold_out, h_hold.data(), n);
  }
  if (rings) {
    ring_fold(chk.data(), rchk.data(), checks_done, check_stride, n, h_ring_checks.data(), rec.ring);
    if (A.ring.out.ring_checks) std::memcpy(A.ring.out.ring_checks, h_ring_checks.data(), 4 * (size_t)n);
  }
  rec.ring.ms_ring = ms_ring; rec.ring.ms_separation = ms_separation; rec.ring.ms_kernels = ms_kernels;
  rec.rol.ms_kernels = ms_kernels; rec.sep.ms_separation = ms_separation;
  rec.rol.ms_total = (float)(1e-3 * (double)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count());
  rec.yld.ms_pair = ms_pair; rec.yld.ms_separation = ms_separation; rec.yld.ms_kernels = ms_kernels; rec.yld.ms_total = rec.rol.ms_total;
  rec.ring.ms_total = rec.rol.ms_total;
  return rc ? rc : rec.sep.checks_skipped ? 2 : 0;
}

int mnav_follow_rollout(mnav_ctx* ctx, uint32_t n, const float* pos, const float* dir, const float* up, const uint32_t* face_in, const uint32_t* slots,
                        const uint32_t* seed_faces, const float* goal_pos, const float* goal_dir, const mnav_follow_config* config,
                        const mnav_rollout_config* rollout, int32_t* status_out, uint32_t* ticks_out, float* pos_out, float* dir_out, uint32_t* face_out,
                        double* travel_out, double* cost_integral_out, float* min_goal_dist_out, float* trace_out)
{
  if (!ctx) return -1;
  return rollout_run(ctx, RolloutCall{ "rollout", &ctx->rol_rec, n, pos, dir, up, face_in, slots, seed_faces, goal_pos, goal_dir, config, rollout, nullptr, nullptr,
                                       { status_out, ticks_out, pos_out, dir_out, face_out, travel_out, cost_integral_out, min_goal_dist_out, trace_out },
                                       mnav_frol::Rows{}, YieldCall{}, RingCall{} });
}

int mnav_fleet_rollout(mnav_ctx* ctx, uint32_t n, const float* pos, const float* dir, const float* up, const uint32_t* face_in, const uint32_t* slots,
                       const uint32_t* seed_faces, const float* goal_pos, const float* goal_dir, const mnav_follow_config* config,
                       const mnav_rollout_config* rollout, const uint32_t* start_tick, const mnav_separation_config* separation, int32_t* status_out,
                       uint32_t* ticks_out, float* pos_out, float* dir_out, uint32_t* face_out, double* travel_out, double* cost_integral_out,
                       float* min_goal_dist_out, float* trace_out, uint32_t* near_checks_out, uint32_t* max_partners_out, uint32_t* first_near_tick_out,
                       uint32_t* first_near_robot_out, float* min_sep2_out, uint32_t* min_sep_tick_out, uint32_t* min_sep_robot_out)
{
  if (!ctx) return -1;
  return rollout_run(ctx, RolloutCall{ "fleet rollout", &ctx->frol_rec, n, pos, dir, up, face_in, slots, seed_faces, goal_pos, goal_dir, config, rollout, start_tick,
                                       separation, { status_out, ticks_out, pos_out, dir_out, face_out, travel_out, cost_integral_out, min_goal_dist_out, trace_out },
                                       { near_checks_out, max_partners_out, first_near_tick_out, first_near_robot_out, min_sep2_out, min_sep_tick_out, min_sep_robot_out },
                                       YieldCall{}, RingCall{} });
}

int mnav_fleet_rollout_yield(mnav_ctx* ctx, uint32_t n, const float* pos, const float* dir, const float* up, const uint32_t* face_in, const uint32_t* slots,
                             const uint32_t* seed_faces, const float* goal_pos, const float* goal_dir, const mnav_follow_config* config,
                             const mnav_rollout_config* rollout, const uint32_t* start_tick, const mnav_separation_config* separation, int32_t* status_out,
                             uint32_t* ticks_out, float* pos_out, float* dir_out, uint32_t* face_out, double* travel_out, double* cost_integral_out,
                             float* min_goal_dist_out, float* trace_out, uint32_t* near_checks_out, uint32_t* max_partners_out, uint32_t* first_near_tick_out,
                             uint32_t* first_near_robot_out, float* min_sep2_out, uint32_t* min_sep_tick_out, uint32_t* min_sep_robot_out,
                             const mnav_yield_config* yield, const uint32_t* priority, const uint8_t* hold_in, uint8_t* hold_out, uint32_t* hold_checks_out,
                             uint32_t* held_ticks_out, uint32_t* first_hold_tick_out, uint32_t* first_hold_robot_out)
{
  if (!ctx) return -1;
  return rollout_run(ctx, RolloutCall{ "fleet rollout yield", &ctx->yld_rec, n, pos, dir, up, face_in, slots, seed_faces, goal_pos, goal_dir, config, rollout, start_tick,
                                       separation, { status_out, ticks_out, pos_out, dir_out, face_out, travel_out, cost_integral_out, min_goal_dist_out, trace_out },
                                       { near_checks_out, max_partners_out, first_near_tick_out, first_near_robot_out, min_sep2_out, min_sep_tick_out, min_sep_robot_out },
                                       YieldCall{ yield, priority, hold_in, hold_out, { hold_checks_out, held_ticks_out, first_hold_tick_out, first_hold_robot_out } },
                                       RingCall{} });
}

int mnav_fleet_rollout_rings(mnav_ctx* ctx, uint32_t n, const float* pos, const float* dir, const float* up, const uint32_t* face_in, const uint32_t* slots,
                             const uint32_t* seed_faces, const float* goal_pos, const float* goal_dir, const mnav_follow_config* config,
                             const mnav_rollout_config* rollout, const uint32_t* start_tick, const mnav_separation_config* separation, int32_t* status_out,
                             uint32_t* ticks_out, float* pos_out, float* dir_out, uint32_t* face_out, double* travel_out, double* cost_integral_out,
                             float* min_goal_dist_out, float* trace_out, uint32_t* near_checks_out, uint32_t* max_partners_out, uint32_t* first_near_tick_out,
                             uint32_t* first_near_robot_out, float* min_sep2_out, uint32_t* min_sep_tick_out, uint32_t* min_sep_robot_out,
                             const mnav_yield_config* yield, const uint32_t* priority, const uint8_t* hold_in, uint8_t* hold_out, uint32_t* hold_checks_out,
                             uint32_t* held_ticks_out, uint32_t* first_hold_tick_out, uint32_t* first_hold_robot_out, const mnav_ring_config* rings,
                             uint8_t* wait_class_out, uint32_t* wait_anchor_out, uint32_t* ring_checks_out, uint32_t* first_ring_tick_out, uint32_t* parked_checks_out,
                             uint32_t* released_checks_out)
{
  if (!ctx) return -1;
  return rollout_run(ctx, RolloutCall{ "fleet rollout rings", &ctx->ring_rec, n, pos, dir, up, face_in, slots, seed_faces, goal_pos, goal_dir, config, rollout, start_tick,
                                       separation, { status_out, ticks_out, pos_out, dir_out, face_out, travel_out, cost_integral_out, min_goal_dist_out, trace_out },
                                       { near_checks_out, max_partners_out, first_near_tick_out, first_near_robot_out, min_sep2_out, min_sep_tick_out, min_sep_robot_out },
                                       YieldCall{ yield, priority, hold_in, hold_out, { hold_checks_out, held_ticks_out, first_hold_tick_out, first_hold_robot_out } },
                                       RingCall{ rings, { ring_checks_out, first_ring_tick_out, parked_checks_out, released_checks_out, wait_class_out, wait_anchor_out } } });
}

// the first eight values of both *_stats functions
static void rollout_stats_get(const mnav_rol::Stats& S, uint32_t* status_counts, uint64_t* robot_ticks, uint64_t* stayed, uint64_t* neighbour, uint64_t* global,
                              uint32_t* built_index, float* ms_kernels, float* ms_total)
{
  if (status_counts) for (int k = 0; k < 4; ++k) status_counts[k] = S.final_status[k];
  if (robot_ticks) *robot_ticks = S.robot_ticks;
  if (stayed) *stayed = S.stayed;
  if (neighbour) *neighbour = S.neighbour;
  if (global) *global = S.global;
  if (built_index) *built_index = S.built_index;
  if (ms_kernels) *ms_kernels = S.ms_kernels;
  if (ms_total) *ms_total = S.ms_total;
}

int mnav_rollout_stats(const mnav_ctx* ctx, uint32_t* status_counts, uint64_t* robot_ticks, uint64_t* stayed, uint64_t* neighbour, uint64_t* global,
                       uint32_t* built_index, float* ms_kernels, float* ms_total)
{
  if (!ctx) return -1;
  rollout_stats_get(ctx->rol_rec.rol, status_counts, robot_ticks, stayed, neighbour, global, built_index, ms_kernels, ms_total);
  return 0;
}

int mnav_fleet_rollout_stats(const mnav_ctx* ctx, uint32_t* status_counts, uint64_t* robot_ticks, uint64_t* stayed, uint64_t* neighbour, uint64_t* global,
                             uint32_t* built_index, uint32_t* checks_run, uint32_t* checks_skipped, uint32_t* first_skipped_tick, uint32_t* robots_near,
                             uint64_t* near_pairs, uint64_t* max_pairs, uint32_t* max_pairs_tick, float* min_sep2, uint32_t* min_pair, uint64_t* tests,
                             uint32_t* max_cell, float* ms_separation, float* ms_kernels, float* ms_total)
{
  if (!ctx) return -1;
  rollout_stats_get(ctx->frol_rec.rol, status_counts, robot_ticks, stayed, neighbour, global, built_index, ms_kernels, ms_total);
  const mnav_frol::SepStats& S = ctx->frol_rec.sep;
  if (checks_run) *checks_run = S.checks_run;
  if (checks_skipped) *checks_skipped = S.checks_skipped;
  if (first_skipped_tick) *first_skipped_tick = S.first_skipped_tick;
  if (robots_near) *robots_near = S.robots_near;
  if (near_pairs) *near_pairs = S.near_pairs;
  if (max_pairs) *max_pairs = S.max_pairs;
  if (max_pairs_tick) *max_pairs_tick = S.max_pairs_tick;
  if (min_sep2) *min_sep2 = S.min_sep2;
  if (min_pair) { min_pair[0] = S.min_pair[0]; min_pair[1] = S.min_pair[1]; }
  if (tests) *tests = S.tests;
  if (max_cell) *max_cell = S.max_cell;
  if (ms_separation) *ms_separation = S.ms_separation;
  return 0;
}

int mnav_fleet_yield_stats(const mnav_ctx* ctx, uint32_t* robots_held, uint64_t* held_ticks, uint32_t* max_held, uint32_t* max_held_tick, uint32_t* held_last,
                           uint32_t* checks_run, uint32_t* checks_skipped, uint32_t* first_skipped_tick, float* ms_pair, float* ms_separation, float* ms_kernels, float* ms_total)
{
  if (!ctx) return -1;
  const mnav_frol::YldStats& S = ctx->yld_rec.yld;
  if (robots_held) *robots_held = S.robots_held;
  if (held_ticks) *held_ticks = S.held_ticks;
  if (max_held) *max_held = S.max_held;
  if (max_held_tick) *max_held_tick = S.max_held_tick;
  if (held_last) *held_last = S.held_last;
  if (checks_run) *checks_run = S.checks_run;
  if (checks_skipped) *checks_skipped = S.checks_skipped;
  if (first_skipped_tick) *first_skipped_tick = S.first_skipped_tick;
  if (ms_pair) *ms_pair = S.ms_pair;
  if (ms_separation) *ms_separation = S.ms_separation;
  if (ms_kernels) *ms_kernels = S.ms_kernels;
  if (ms_total) *ms_total = S.ms_total;
  return 0;
}

int mnav_fleet_ring_stats(const mnav_ctx* ctx, uint32_t* robots_ring, uint64_t* rings, uint32_t* max_rings, uint32_t* max_rings_tick, uint64_t* releases,
                          uint32_t* members_last, uint32_t* tails_last, uint32_t* parked_last, uint32_t* queued_last, uint32_t* rings_last, uint32_t* checks_run,
                          uint32_t* checks_skipped, uint32_t* first_skipped_tick, float* ms_ring, float* ms_separation, float* ms_kernels, float* ms_total)
{
  if (!ctx) return -1;
  const mnav_frol::RingStats& S = ctx->ring_rec.ring;
  if (robots_ring) *robots_ring = S.robots_ring;
  if (rings) *rings = S.rings;
  if (max_rings) *max_rings = S.max_rings;
  if (max_rings_tick) *max_rings_tick = S.max_rings_tick;
  if (releases) *releases = S.releases;
  if (members_last) *members_last = S.members_last;
  if (tails_last) *tails_last = S.tails_last;
  if (parked_last) *parked_last = S.parked_last;
  if (queued_last) *queued_last = S.queued_last;
  if (rings_last) *rings_last = S.rings_last;
  if (checks_run) *checks_run = S.checks_run;
  if (checks_skipped) *checks_skipped = S.checks_skipped;
  if (first_skipped_tick) *first_skipped_tick = S.first_skipped_tick;
  if (ms_ring) *ms_ring = S.ms_ring;
  if (ms_separation) *ms_separation = S.ms_separation;
  if (ms_kernels) *ms_kernels = S.ms_kernels;
  if (ms_total) *ms_total = S.ms_total;
  return 0;
}
