// mnav_timed_capi.h -- the C ABI of timed fleet traffic (include/mnav.h: mnav_fleet_timed_traffic,
// mnav_timed_traffic_download, mnav_timed_traffic_stats, mnav_layer_timed_traffic, mnav_map_timed_traffic) over the kernels
// of mnav_timed.h, the shared steps of mnav_fleet_capi.h, layer_change_list and map_propagate.  Included by mnav.hip inside
// its extern "C" block, after mnav_traffic_capi.h (FleetStatsKeep, traffic_check_args).
#pragma once

constexpr double kTimedTrafficMaxMb = 2048.0;   // default of the option timed_traffic_max_mb

// peak (zero when new), first window (MNAV_NONE when new) and the counters
static int timed_reserve_peak(mnav_ctx* ctx)
{
  using namespace mnav_timed;
  State& T = ctx->timed;
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  if (!T.peak) {
    const size_t V = ctx->V ? ctx->V : 1;
    if (alloc_group(T.peak, 4 * V, T.window, 4 * V, T.words, sizeof(unsigned long long) * kWords) != hipSuccess) {
      ctx->err = "timed traffic: out of device memory"; return -1;
    }
    HIPCHK(hipMemsetAsync(T.peak, 0, 4 * V, ctx->stream));
    HIPCHK(hipMemsetAsync(T.window, 0xFF, 4 * V, ctx->stream));
  }
  return 0;
}

// cells and holders of B windows (*fresh: they are new and hold nothing yet), room for n robots
static int timed_reserve(mnav_ctx* ctx, size_t n, uint32_t B, bool* fresh)
{
  using namespace mnav_timed;
  State& T = ctx->timed;
  if (timed_reserve_peak(ctx)) return -1;
  *fresh = false;
  if (T.B != B || !T.cell) {
    const size_t cells = (size_t)(ctx->V ? ctx->V : 1) * B;
    T.B = 0; T.T = 0ull;
    if (alloc_group(T.cell, 4 * cells, T.holder, 4 * cells) != hipSuccess) { ctx->err = "timed traffic: out of device memory"; return -1; }
    T.B = B; *fresh = true;
  }
  if (n > T.cap) {
    T.cap = 0;
    if (alloc_group(T.weight, 4 * n, T.key, 4 * n, T.conflict, 4 * n, T.yield, 4 * n, T.fy_vertex, 4 * n, T.fy_window, 4 * n, T.depart, 4 * n, T.pace, 4 * n,
                    T.fy_time, 4 * n) != hipSuccess) { ctx->err = "timed traffic: out of device memory"; return -1; }
    T.cap = n;
  }
  return 0;
}

int mnav_fleet_timed_traffic(mnav_ctx* ctx, uint32_t n, const uint32_t* slots, const uint32_t* start_vertex, const float* start_pos, const uint32_t* weights,
                             const float* depart, const float* pace, const uint32_t* key, uint32_t windows, double tau, uint32_t free_count, int accumulate,
                             uint32_t* code_out, uint32_t* vertex_out, float* potential_out, uint32_t* conflict_hops_out, uint32_t* yield_hops_out,
                             uint32_t* first_yield_vertex_out, uint32_t* first_yield_window_out, float* first_yield_time_out)
{
  using namespace mnav_timed;
  if (!ctx) return -1;
  ctx->err.clear();
  if (!n && accumulate) return 0;                                     // (n = 0 without `accumulate` still starts the cells over)
  const auto t0 = std::chrono::steady_clock::now();
  // every refusal comes before the first device call: a refused call touches nothing
  if (n && !slots) { ctx->err = "fleet timed traffic: null slots"; return -1; }
  if (n && !start_vertex && !start_pos) { ctx->err = "fleet timed traffic: neither start vertices nor start positions"; return -1; }
  std::vector<mnav_fleet::Field> fields;
  if (fleet_fields_of(ctx, "fleet timed traffic", n, slots, fields)) return -1;
  State& T = ctx->timed;
  const uint32_t B = windows, V = ctx->V;
  if (const char* why = timed_refusal(n, weights, depart, pace, B, tau, accumulate, T.T, T.cell ? T.B : 0u, T.tau)) {
    ctx->err = std::string("fleet timed traffic: ") + why; return -1;
  }
  const double mb = opt_set(ctx->opt.timed_traffic_max_mb) ? std::max(ctx->opt.timed_traffic_max_mb, 0.0) : kTimedTrafficMaxMb;
  if (8.0 * (double)(V ? V : 1) * (double)B > mb * 1048576.0) { ctx->err = "fleet timed traffic: cells and holders are larger than timed_traffic_max_mb"; return -1; }
  FleetStatsKeep keep(ctx->fleet);
  bool fresh = false;
  if (timed_reserve(ctx, n, B, &fresh)) return -1;
  const size_t cells = (size_t)(V ? V : 1) * B;
  if (!accumulate || fresh) {
    HIPCHK(hipMemsetAsync(T.cell, 0, 4 * cells, ctx->stream));
    HIPCHK(hipMemsetAsync(T.holder, 0xFF, 4 * cells, ctx->stream));
    T.T = 0ull; T.tau = (float)tau;
  }
  HIPCHK(hipMemsetAsync(T.words, 0, sizeof(unsigned long long) * kWords, ctx->stream));
  T.contributing = T.adds = T.beyond = 0; T.built_index = 0; T.ms_kernels = 0.f;
  mnav_fleet::State& S = ctx->fleet;
  uint32_t G = 1u;
  while (G < B && G < 64u) G <<= 1;                                   // lanes per vertex of the peak pass
  const uint32_t peak_blocks = (uint32_t)std::min<size_t>(((size_t)V * G + kTimedBlock - 1) / kTimedBlock, std::max(1u, opt_u32(ctx->opt.timed_peak_blocks, kPeakBlocks)));
  if (n) {
    if (weights) HIPCHK(hipMemcpyAsync(T.weight, weights, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if (depart) HIPCHK(hipMemcpyAsync(T.depart, depart, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if (pace) HIPCHK(hipMemcpyAsync(T.pace, pace, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if (key) HIPCHK(hipMemcpyAsync(T.key, key, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    mnav_fleet::Paths P{};
    const uint32_t* d_vtx = nullptr;
    if (fleet_classify_robots(ctx, n, slots, start_vertex, start_pos, fields, P, &d_vtx)) return -1;
    T.built_index = S.built_index;
    Walk A{};
    A.n = n; A.V = V; A.B = B; A.tau = T.tau; A.free_count = free_count;
    A.slot = P.slot; A.vtx = P.vtx; A.fields = P.fields; A.code = P.code; A.len = P.len; A.potential = P.potential;
    A.weight = weights ? T.weight.get() : (const uint32_t*)nullptr; A.depart = depart ? T.depart.get() : (const float*)nullptr;
    A.pace = pace ? T.pace.get() : (const float*)nullptr; A.key = key ? T.key.get() : (const uint32_t*)nullptr;
    A.cell = T.cell; A.holder = T.holder; A.words = T.words;
    A.conflict = T.conflict; A.yield = T.yield; A.fy_vertex = T.fy_vertex; A.fy_window = T.fy_window; A.fy_time = T.fy_time;
    const dim3 grid((n + kTimedBlock - 1) / kTimedBlock);
    hipLaunchKernelGGL(k_timed_add, grid, dim3(kTimedBlock), 0, ctx->stream, A);
    if (V) hipLaunchKernelGGL(k_timed_peak, dim3(peak_blocks), dim3(kTimedBlock), 0, ctx->stream, V, B, G, free_count, T.cell.get(), T.peak.get(), T.window.get(), T.words.get());
    hipLaunchKernelGGL(k_timed_report, grid, dim3(kTimedBlock), 0, ctx->stream, A);   // after every add: the kernel boundary orders the reads
    unsigned long long unused = 0; uint32_t cnt[mnav_fleet::kCounters + 1] = {};     // (no scan ran: the hop total is not this call's)
    if (fleet_finish_classify(ctx, P, fields.size(), &unused, cnt)) return -1;
    T.ms_kernels = S.ms_kernels;
    if (code_out) HIPCHK(hipMemcpyAsync(code_out, S.code, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (vertex_out) HIPCHK(hipMemcpyAsync(vertex_out, d_vtx, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (potential_out) HIPCHK(hipMemcpyAsync(potential_out, S.potential, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (conflict_hops_out) HIPCHK(hipMemcpyAsync(conflict_hops_out, T.conflict, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (yield_hops_out) HIPCHK(hipMemcpyAsync(yield_hops_out, T.yield, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (first_yield_vertex_out) HIPCHK(hipMemcpyAsync(first_yield_vertex_out, T.fy_vertex, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (first_yield_window_out) HIPCHK(hipMemcpyAsync(first_yield_window_out, T.fy_window, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (first_yield_time_out) HIPCHK(hipMemcpyAsync(first_yield_time_out, T.fy_time, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  } else if (V) {
    hipLaunchKernelGGL(k_timed_peak, dim3(peak_blocks), dim3(kTimedBlock), 0, ctx->stream, V, B, G, free_count, T.cell.get(), T.peak.get(), T.window.get(), T.words.get());
    HIPCHK(hipGetLastError());
  }
  unsigned long long words[kWords] = {};
  HIPCHK(hipMemcpyAsync(words, T.words, sizeof(words), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  T.T += words[kWeight];
  T.contributing = words[kContributing]; T.adds = words[kAdds]; T.beyond = words[kBeyond];
  T.occupied = words[kOccupied]; T.over = words[kOver]; T.largest = (uint32_t)words[kLargest]; T.yielding = (uint32_t)words[kYielding];
  T.windows = B;
  T.ms_total = (float)(1e-3 * (double)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count());
  return 0;
}

int mnav_timed_traffic_download(const mnav_ctx* cctx, uint32_t* peak_out, uint32_t* window_out, uint32_t* cells_out, uint32_t* holders_out)
{
  if (!cctx) return -1;
  mnav_ctx* ctx = const_cast<mnav_ctx*>(cctx);                      // the error string and the stream are the context's
  ctx->err.clear();
  if (!ctx->have_mesh) { ctx->err = "mnav_upload_mesh has not been called"; return -1; }
  const mnav_timed::State& T = ctx->timed;
  const size_t V = ctx->V;
  if (!T.peak) {                                                      // no timed call since the mesh: zero peaks, no window, no cells
    if (peak_out) memset(peak_out, 0, 4 * V);
    if (window_out) memset(window_out, 0xFF, 4 * V);
    return 0;
  }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  if (V) {
    if (peak_out) HIPCHK(hipMemcpyAsync(peak_out, T.peak, 4 * V, hipMemcpyDeviceToHost, ctx->stream));
    if (window_out) HIPCHK(hipMemcpyAsync(window_out, T.window, 4 * V, hipMemcpyDeviceToHost, ctx->stream));
    if (T.cell && T.B) {
      if (cells_out) HIPCHK(hipMemcpyAsync(cells_out, T.cell, 4 * V * T.B, hipMemcpyDeviceToHost, ctx->stream));
      if (holders_out) HIPCHK(hipMemcpyAsync(holders_out, T.holder, 4 * V * T.B, hipMemcpyDeviceToHost, ctx->stream));
    }
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mnav_timed_traffic_stats(const mnav_ctx* ctx, uint32_t* contributing, uint64_t* adds, uint64_t* beyond_horizon, uint64_t* total_weight,
                             uint64_t* occupied_cells, uint64_t* over_cells, uint32_t* largest_cell, uint32_t* yielding, uint32_t* windows,
                             uint32_t* built_index, float* ms_kernels, float* ms_total)
{
  if (!ctx) return -1;
  const mnav_timed::State& T = ctx->timed;
  if (contributing) *contributing = (uint32_t)T.contributing;
  if (adds) *adds = T.adds;
  if (beyond_horizon) *beyond_horizon = T.beyond;
  if (total_weight) *total_weight = T.T;
  if (occupied_cells) *occupied_cells = T.occupied;
  if (over_cells) *over_cells = T.over;
  if (largest_cell) *largest_cell = T.largest;
  if (yielding) *yielding = T.yielding;
  if (windows) *windows = T.windows;
  if (built_index) *built_index = T.built_index;
  if (ms_kernels) *ms_kernels = T.ms_kernels;
  if (ms_total) *ms_total = T.ms_total;
  return 0;
}

int mnav_layer_timed_traffic(mnav_ctx* ctx, uint32_t layer, uint32_t free_count, double gain, double cap, uint32_t* changed_out, uint32_t* n_changed)
{
  using namespace mnav_traffic;
  if (!ctx) return -1;
  ctx->err.clear();
  if (traffic_check_args(ctx, gain, cap)) return -1;
  if (layer_slot(ctx, layer, false)) return -1;
  if (timed_reserve_peak(ctx)) return -1;
  uint32_t c[mnav_chg::kCounters];
  const TrafficRule rule{ ctx->timed.peak, free_count, (float)gain, (float)cap };   // the traffic rule on the peaks
  return layer_change_list(ctx, ctx->layers[layer], rule, ctx->ev[7], c, changed_out, n_changed, nullptr);
}

int mnav_map_timed_traffic(mnav_ctx* ctx, uint32_t layer, uint32_t free_count, double gain, double cap, uint32_t* changed_out, uint32_t* n_changed)
{
  using namespace mnav_map;
  if (!ctx) return -1;
  ctx->err.clear();
  if (map_update_ready(ctx, layer, true)) return -1;
  if (traffic_check_args(ctx, gain, cap)) return -1;                // (the graph stays usable)
  State& S = ctx->map;
  HIPCHK(hipEventRecord(S.ev[0], ctx->stream));
  uint32_t nc = 0;
  // the writer leaves its list (the vertices whose cost bits or flag changed) in the change-list scratch: it stays there
  if (mnav_layer_timed_traffic(ctx, layer, free_count, gain, cap, nullptr, &nc)) return map_finish(ctx, -1);
  Node& src = S.order[S.pos[layer]];
  src.out = ctx->chg.ids; src.n_out = nc; src.flipped = nc;          // (the slot may have held lethal flags: assume some flipped)
  return map_finish(ctx, map_propagate(ctx, (uint32_t)S.pos[layer], changed_out, n_changed));
}
