// mnav_timed_capi.h -- the C ABI of timed fleet traffic (include/mnav.h: mnav_fleet_timed_traffic,
// mnav_timed_traffic_download, mnav_timed_traffic_stats, mnav_layer_timed_traffic, mnav_map_timed_traffic) over the kernels
// of mnav_timed.h, the FleetCall of mnav_fleet_capi.h and the layer and map bodies of mnav_traffic_capi.h.  TimedCells and
// timed_peak state the life of the cells through a call once, for this call and for mnav_schedule_capi.h.  Included by
// mnav.hip inside its extern "C" block, after mnav_traffic_capi.h.
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

// The timed cells through one call that adds to them (mnav_fleet_timed_traffic, mnav_fleet_schedule), in this order:
// too_large (a refusal: before anything is touched), reserve, reset, upload, the caller's kernels with timed_peak after the
// last add, read_words.  A caller with arrays of its own per cell reserves them between reserve and reset.
struct TimedCells {
  mnav_ctx* ctx; uint32_t n, B; double tau; int accumulate;
  bool fresh = false; unsigned long long words[mnav_timed::kWords] = {};
  const uint32_t* weight = nullptr; const float* depart = nullptr; const float* pace = nullptr; const uint32_t* key = nullptr;   // on the device, null: not given

  size_t cells() const { return (size_t)(ctx->V ? ctx->V : 1) * B; }
  // `text`: the whole message, it names what the caller keeps per cell
  int too_large(double bytes_per_cell, const char* text) const
  {
    const double mb = opt_set(ctx->opt.timed_traffic_max_mb) ? std::max(ctx->opt.timed_traffic_max_mb, 0.0) : kTimedTrafficMaxMb;
    if (bytes_per_cell * (double)(ctx->V ? ctx->V : 1) * (double)B > mb * 1048576.0) { ctx->err = text; return -1; }
    return 0;
  }

  // cells and holders of B windows (fresh: they are new and hold nothing yet), room for n robots
  int reserve()
  {
    mnav_timed::State& T = ctx->timed;
    if (timed_reserve_peak(ctx)) return -1;
    if (T.B != B || !T.cell) {
      T.B = 0; T.T = 0ull;
      if (alloc_group(T.cell, 4 * cells(), T.holder, 4 * cells()) != hipSuccess) { ctx->err = "timed traffic: out of device memory"; return -1; }
      T.B = B; fresh = true;
    }
    if (n > T.cap) {
      T.cap = 0;
      const size_t b = 4 * (size_t)n;
      if (alloc_group(T.weight, b, T.key, b, T.conflict, b, T.yield, b, T.fy_vertex, b, T.fy_window, b, T.depart, b, T.pace, b, T.fy_time, b) != hipSuccess) {
        ctx->err = "timed traffic: out of device memory"; return -1;
      }
      T.cap = n;
    }
    return 0;
  }

  // the cells start over unless the call accumulates on cells that hold something; the words and the call's statistics always do
  int reset()
  {
    using namespace mnav_timed;
    State& T = ctx->timed;
    if (!accumulate || fresh) {
      HIPCHK(hipMemsetAsync(T.cell, 0, 4 * cells(), ctx->stream));
      HIPCHK(hipMemsetAsync(T.holder, 0xFF, 4 * cells(), ctx->stream));
      T.T = 0ull; T.tau = (float)tau;
    }
    HIPCHK(hipMemsetAsync(T.words, 0, sizeof(unsigned long long) * kWords, ctx->stream));
    T.contributing = T.adds = T.beyond = 0; T.built_index = 0; T.ms_kernels = 0.f;
    return 0;
  }

  // the optional arrays per robot (n > 0)
  int upload(const uint32_t* weights, const float* h_depart, const float* h_pace, const uint32_t* h_key)
  {
    mnav_timed::State& T = ctx->timed;
    const size_t bytes = 4 * (size_t)n;
    if (weights) { HIPCHK(hipMemcpyAsync(T.weight, weights, bytes, hipMemcpyHostToDevice, ctx->stream)); weight = T.weight; }
    if (h_depart) { HIPCHK(hipMemcpyAsync(T.depart, h_depart, bytes, hipMemcpyHostToDevice, ctx->stream)); depart = T.depart; }
    if (h_pace) { HIPCHK(hipMemcpyAsync(T.pace, h_pace, bytes, hipMemcpyHostToDevice, ctx->stream)); pace = T.pace; }
    if (h_key) { HIPCHK(hipMemcpyAsync(T.key, h_key, bytes, hipMemcpyHostToDevice, ctx->stream)); key = T.key; }
    return 0;
  }

  // the words of the peak pass come down (the call's last wait) with what they tell of the cells
  int read_words()
  {
    using namespace mnav_timed;
    State& T = ctx->timed;
    HIPCHK(hipMemcpyAsync(words, T.words, sizeof(words), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    T.occupied = words[kOccupied]; T.over = words[kOver]; T.largest = (uint32_t)words[kLargest]; T.windows = B;
    return 0;
  }
};

// the robots and the cells as a kernel's argument record names them (mnav_timed::Walk, mnav_schedule::Job)
extern "C++" {
template <class Args>
static void timed_fill(Args& A, const TimedCells& C, const FleetCall& R)
{
  fleet_fill(A, R, C.weight);
  A.B = C.B; A.tau = C.ctx->timed.tau; A.depart = C.depart; A.pace = C.pace; A.key = C.key; A.cell = C.ctx->timed.cell; A.holder = C.ctx->timed.holder;
}
}  // extern "C++"

// peak, first window over `threshold` and the cell statistics from the cells as they stand
static int timed_peak(mnav_ctx* ctx, uint32_t B, uint32_t threshold)
{
  using namespace mnav_timed;
  State& T = ctx->timed;
  const uint32_t V = ctx->V;
  if (!V) return 0;
  uint32_t G = 1u;
  while (G < B && G < 64u) G <<= 1;                                   // lanes per vertex of the peak pass
  const uint32_t peak_blocks = (uint32_t)std::min<size_t>(((size_t)V * G + kTimedBlock - 1) / kTimedBlock, std::max(1u, opt_u32(ctx->opt.timed_peak_blocks, kPeakBlocks)));
  hipLaunchKernelGGL(k_timed_peak, dim3(peak_blocks), dim3(kTimedBlock), 0, ctx->stream, V, B, G, threshold, T.cell.get(), T.peak.get(), T.window.get(), T.words.get());
  HIPCHK(hipGetLastError());
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
  FleetCall R{ ctx, "fleet timed traffic", n, slots, start_vertex, start_pos };
  if (R.begin()) return -1;
  State& T = ctx->timed;
  TimedCells C{ ctx, n, windows, tau, accumulate };
  if (const char* why = timed_refusal(n, weights, depart, pace, C.B, tau, accumulate, T.T, T.cell ? T.B : 0u, T.tau)) {
    ctx->err = std::string("fleet timed traffic: ") + why; return -1;
  }
  if (C.too_large(8.0, "fleet timed traffic: cells and holders are larger than timed_traffic_max_mb")) return -1;
  FleetStatsKeep keep(ctx->fleet);
  if (C.reserve() || C.reset()) return -1;
  if (n) {
    if (C.upload(weights, depart, pace, key) || R.classify()) return -1;
    T.built_index = ctx->fleet.stats.built_index;
    Walk A{};
    timed_fill(A, C, R);
    A.free_count = free_count; A.words = T.words;
    A.conflict = T.conflict; A.yield = T.yield; A.fy_vertex = T.fy_vertex; A.fy_window = T.fy_window; A.fy_time = T.fy_time;
    const dim3 grid((n + kTimedBlock - 1) / kTimedBlock);
    hipLaunchKernelGGL(k_timed_add, grid, dim3(kTimedBlock), 0, ctx->stream, A);
    if (timed_peak(ctx, C.B, free_count)) return -1;
    hipLaunchKernelGGL(k_timed_report, grid, dim3(kTimedBlock), 0, ctx->stream, A);   // after every add: the kernel boundary orders the reads
    if (R.finish()) return -1;
    T.ms_kernels = ctx->fleet.stats.ms_kernels;
    if (R.download(code_out, vertex_out, potential_out)) return -1;
    if (conflict_hops_out) HIPCHK(hipMemcpyAsync(conflict_hops_out, T.conflict, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (yield_hops_out) HIPCHK(hipMemcpyAsync(yield_hops_out, T.yield, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (first_yield_vertex_out) HIPCHK(hipMemcpyAsync(first_yield_vertex_out, T.fy_vertex, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (first_yield_window_out) HIPCHK(hipMemcpyAsync(first_yield_window_out, T.fy_window, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (first_yield_time_out) HIPCHK(hipMemcpyAsync(first_yield_time_out, T.fy_time, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  } else if (timed_peak(ctx, C.B, free_count)) return -1;
  if (C.read_words()) return -1;
  T.T += C.words[kWeight];
  T.contributing = C.words[kContributing]; T.adds = C.words[kAdds]; T.beyond = C.words[kBeyond]; T.yielding = (uint32_t)C.words[kYielding];
  T.ms_total = R.ms_total();
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
  return traffic_layer_run(ctx, true, layer, free_count, gain, cap, changed_out, n_changed);   // the traffic rule on the peaks
}

int mnav_map_timed_traffic(mnav_ctx* ctx, uint32_t layer, uint32_t free_count, double gain, double cap, uint32_t* changed_out, uint32_t* n_changed)
{
  return traffic_map_run(ctx, true, layer, free_count, gain, cap, changed_out, n_changed);
}
