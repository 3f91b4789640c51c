// mnav_rollout_capi.h -- the C ABI of the device rollout (include/mnav.h: mnav_follow_rollout, mnav_rollout_stats) over
// the kernels of mnav_rollout.h.  Included by mnav.hip inside its extern "C" block, after mnav_follow_capi.h (the argument
// checks are the follower's) and mnav_locate_capi.h (the index build is the lookup's own).
#pragma once

static int rollout_reserve(mnav_ctx* ctx, size_t n, bool goals, size_t ticks, size_t trace_floats)
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
    if (S.cnt.alloc(sizeof(uint32_t) * mnav_rol::kCounters * ticks) != hipSuccess) { ctx->err = oom; return -1; }
    S.cnt_cap = ticks;
  }
  if (trace_floats > S.trace_cap) {
    S.trace_cap = 0;
    if (S.trace.alloc(sizeof(float) * trace_floats) != hipSuccess) { ctx->err = oom; return -1; }
    S.trace_cap = trace_floats;
  }
  return 0;
}

// The argument checks of a rollout beside the follower's (mnav_follow_rollout, mnav_fleet_rollout), all on the host: -1 with
// ctx->err set, or 0.
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

int mnav_follow_rollout(mnav_ctx* ctx, uint32_t n, const float* pos, const float* dir, const float* up, const uint32_t* face_in, const uint32_t* slots,
                        const uint32_t* seed_faces, const float* goal_pos, const float* goal_dir, const mnav_follow_config* config,
                        const mnav_rollout_config* rollout, int32_t* status_out, uint32_t* ticks_out, float* pos_out, float* dir_out, uint32_t* face_out,
                        double* travel_out, double* cost_integral_out, float* min_goal_dist_out, float* trace_out)
{
  using namespace mnav_rol;
  if (!ctx) return -1;
  ctx->err.clear();
  if (!n) return 0;
  const auto t0 = std::chrono::steady_clock::now();
  // every refusal comes before the first device call: a refused call touches nothing
  std::vector<const float*> maps;
  if (follow_check(ctx, n, pos, dir, up, face_in, slots, seed_faces, config, maps)) return -1;
  if (rollout_check(ctx, goal_pos, goal_dir, config, rollout, trace_out)) return -1;
  const uint32_t ticks = rollout->ticks, stride = rollout->trace_stride, rows = stride ? ticks / stride : 0;
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  cancel_reset(ctx);                                                  // as the plan calls do
  if (upload_walk_mesh(ctx)) return -1;
  if (staging_reserve(ctx, n, ctx->res.plans(), "rollout") || rollout_reserve(ctx, n, goal_pos != nullptr, ticks, 3 * (size_t)n * rows)) return -1;
  Dev& S = ctx->rol;
  mnav_fol::Staging& G = ctx->stage;
  for (auto& c : S.final_status) c = 0;
  S.built_index = 0; S.robot_ticks = S.stayed = S.neighbour = S.global = 0; S.ms_kernels = S.ms_total = 0.f;
  if (locate_ensure(ctx, &S.built_index)) return -1;                  // no look at the lists between ticks: the index exists before the first one
  const mnav_loc::State& L = ctx->loc;
  Batch B{};
  if (staging_upload(ctx, n, pos, dir, up, face_in, slots, seed_faces, maps, B)) return -1;
  if (goal_pos) {
    HIPCHK(hipMemcpyAsync(S.goal_pos, goal_pos, 12 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(S.goal_dir, goal_dir, 12 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  }
  HIPCHK(hipMemsetAsync(S.status, 0, 4 * (size_t)n, ctx->stream));    // kRunning
  HIPCHK(hipMemsetAsync(S.ticks, 0, 4 * (size_t)n, ctx->stream));
  HIPCHK(hipMemsetAsync(S.travel, 0, 8 * (size_t)n, ctx->stream));
  HIPCHK(hipMemsetAsync(S.cost_integral, 0, 8 * (size_t)n, ctx->stream));
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)S.min_goal_dist.get(), 0x7F800000, n, ctx->stream));   // +inf
  HIPCHK(hipMemsetAsync(S.cnt, 0, sizeof(uint32_t) * kCounters * (size_t)ticks, ctx->stream));    // every tick's row, once
  B.pos = G.pos; B.dir = G.dir; B.up = G.up; B.face = G.face; B.cnt = S.cnt;
  B.status = S.status; B.ticks = S.ticks; B.travel = S.travel; B.cost_integral = S.cost_integral; B.min_goal_dist = S.min_goal_dist;
  B.goal_pos = goal_pos ? S.goal_pos.get() : nullptr; B.goal_dir = goal_pos ? S.goal_dir.get() : nullptr;
  B.trace = rows ? S.trace.get() : nullptr; B.trace_rows = rows;
  mnav_fol::Config C;
  std::memcpy(&C, config, sizeof(C));
  const Params P{ rollout->dt, (float)rollout->dist_tolerance, (float)rollout->angle_tolerance, goal_pos != nullptr };
  const WalkMesh M{ ctx->d_xyz, ctx->d_faces, ctx->d_vf_ptr, ctx->d_vf, ctx->V, ctx->F };
  const mnav_loc::Index I{ L.nodes, L.pts, L.n_pts, L.n_leaves, mnav_loc::loc_root(L.n_leaves) };
  const uint32_t g_stay = (n + kStayBlock - 1) / kStayBlock, g_search = n < 2048u ? n : 2048u;
  const uint32_t g_all = (n + mnav_loc::kLocBlock - 1) / mnav_loc::kLocBlock, g_global = g_all < 1024u ? g_all : 1024u;
  float ms_kernels = 0.f;
  // one block: plain launches, no host look in between; then one synchronise
  const auto run_block = [&](uint32_t first, uint32_t nt) -> int {
    HIPCHK(hipEventRecord(G.ev[0], ctx->stream));
    for (uint32_t t = first; t < first + nt; ++t) {
      const uint32_t row = stride && (t + 1) % stride == 0 ? (t + 1) / stride - 1 : kNone;
      hipLaunchKernelGGL(k_rollout_stay, dim3(g_stay), dim3(kStayBlock), 0, ctx->stream, B, M, C, P, t, row);
      hipLaunchKernelGGL(k_rollout_search, dim3(g_search), dim3(64), 0, ctx->stream, B, M, C, P, t, row);
      hipLaunchKernelGGL(k_rollout_global, dim3(g_global), dim3(mnav_loc::kLocBlock), 0, ctx->stream, B, M, C, P, I, t, row);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(G.ev[1], ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ms_kernels += ev_ms(G.ev[0], G.ev[1]);
    return 0;
  };
  uint32_t done = 0;
  const int rc = rol_blocks(ticks, run_block, [&] { return ctx->cancel.load(std::memory_order_relaxed) != 0; }, &done);
  if (rc < 0) return -1;
  std::vector<uint32_t> cnt((size_t)kCounters * done);
  HIPCHK(hipMemcpyAsync(cnt.data(), S.cnt, sizeof(uint32_t) * cnt.size(), hipMemcpyDeviceToHost, ctx->stream));
  if (status_out) HIPCHK(hipMemcpyAsync(status_out, S.status, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (ticks_out) HIPCHK(hipMemcpyAsync(ticks_out, S.ticks, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (pos_out) HIPCHK(hipMemcpyAsync(pos_out, G.pos, 12 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (dir_out) HIPCHK(hipMemcpyAsync(dir_out, G.dir, 12 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (face_out) HIPCHK(hipMemcpyAsync(face_out, G.face, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (travel_out) HIPCHK(hipMemcpyAsync(travel_out, S.travel, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (cost_integral_out) HIPCHK(hipMemcpyAsync(cost_integral_out, S.cost_integral, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (min_goal_dist_out) HIPCHK(hipMemcpyAsync(min_goal_dist_out, S.min_goal_dist, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (rows) HIPCHK(hipMemcpyAsync(trace_out, S.trace, 12 * (size_t)n * rows, hipMemcpyDeviceToHost, ctx->stream));   // (rows past a cancel are not written)
  HIPCHK(hipStreamSynchronize(ctx->stream));
  uint64_t sum[kCounters] = {};
  for (size_t t = 0; t < done; ++t)
    for (int k = 2; k < kCounters; ++k) sum[k] += cnt[(size_t)kCounters * t + k];
  S.stayed = sum[2]; S.neighbour = sum[3]; S.global = sum[4];
  S.final_status[kReached] = (uint32_t)sum[5]; S.final_status[kOutOfMap] = (uint32_t)sum[6]; S.final_status[kNoField] = (uint32_t)sum[7];
  S.final_status[kRunning] = n - (uint32_t)(sum[5] + sum[6] + sum[7]);
  S.robot_ticks = sum[2] + sum[3] + sum[4] + sum[6];                  // every tick of a robot ends in a face or out of the map
  S.ms_kernels = ms_kernels;
  S.ms_total = (float)(1e-3 * (double)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count());
  return rc;
}

int mnav_rollout_stats(const mnav_ctx* ctx, uint32_t* status_counts, uint64_t* robot_ticks, uint64_t* stayed, uint64_t* neighbour, uint64_t* global,
                       uint32_t* built_index, float* ms_kernels, float* ms_total)
{
  if (!ctx) return -1;
  const mnav_rol::Dev& S = ctx->rol;
  if (status_counts) for (int k = 0; k < 4; ++k) status_counts[k] = S.final_status[k];
  if (robot_ticks) *robot_ticks = S.robot_ticks;
  if (stayed) *stayed = S.stayed;
  if (neighbour) *neighbour = S.neighbour;
  if (global) *global = S.global;
  if (built_index) *built_index = S.built_index;
  if (ms_kernels) *ms_kernels = S.ms_kernels;
  if (ms_total) *ms_total = S.ms_total;
  return 0;
}
