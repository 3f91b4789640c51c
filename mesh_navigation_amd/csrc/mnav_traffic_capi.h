// mnav_traffic_capi.h -- the C ABI of fleet traffic (include/mnav.h: mnav_fleet_traffic, mnav_traffic_download,
// mnav_traffic_stats, mnav_layer_traffic, mnav_map_traffic) over the kernels of mnav_traffic.h, the FleetCall of
// mnav_fleet_capi.h, layer_change_list and map_propagate; traffic_layer_run and traffic_map_run also serve the timed pair of
// mnav_timed_capi.h.  Included by mnav.hip inside its extern "C" block, after mnav_dispatch_capi.h.
#pragma once

// the counts (zero when they are new), the counters and room for n weights
static int traffic_reserve(mnav_ctx* ctx, size_t n)
{
  using namespace mnav_traffic;
  State& T = ctx->traffic;
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  if (!T.c) {
    const size_t V = ctx->V ? ctx->V : 1;
    if (alloc_group(T.c, 4 * V, T.sums, sizeof(unsigned long long) * kSums, T.vstat, sizeof(uint32_t) * kVertexStats) != hipSuccess) {
      ctx->err = "fleet traffic: out of device memory"; return -1;
    }
    HIPCHK(hipMemsetAsync(T.c, 0, 4 * V, ctx->stream));
    T.T = 0ull;
  }
  if (n > T.cap) {
    T.cap = 0;
    if (T.weight.alloc(4 * n) != hipSuccess) { ctx->err = "fleet traffic: out of device memory"; return -1; }
    T.cap = n;
  }
  return 0;
}

int mnav_fleet_traffic(mnav_ctx* ctx, uint32_t n, const uint32_t* slots, const uint32_t* start_vertex, const float* start_pos, const uint32_t* weights,
                       int accumulate, uint32_t* code_out, uint32_t* vertex_out, float* potential_out)
{
  using namespace mnav_traffic;
  if (!ctx) return -1;
  ctx->err.clear();
  if (!n && accumulate) return 0;                                     // (n = 0 without `accumulate` still starts the counts over)
  FleetCall R{ ctx, "fleet traffic", n, slots, start_vertex, start_pos };
  if (R.begin()) return -1;
  State& T = ctx->traffic;
  unsigned long long all = accumulate ? T.T : 0ull;
  if (weights) for (uint32_t i = 0; i < n; ++i) all += weights[i];
  else all += n;
  if (all > kMaxTotal) { ctx->err = "fleet traffic: total weight does not fit the counters"; return -1; }
  FleetStatsKeep keep(ctx->fleet);
  if (traffic_reserve(ctx, n)) return -1;
  const uint32_t V = ctx->V;
  if (!accumulate) { HIPCHK(hipMemsetAsync(T.c, 0, 4 * (size_t)(V ? V : 1), ctx->stream)); T.T = 0ull; }
  HIPCHK(hipMemsetAsync(T.sums, 0, sizeof(unsigned long long) * kSums, ctx->stream));
  HIPCHK(hipMemsetAsync(T.vstat, 0, sizeof(uint32_t) * kVertexStats, ctx->stream));
  T.contributing = T.built_index = 0; T.adds = 0; T.ms_kernels = 0.f;
  if (n) {
    if (weights) HIPCHK(hipMemcpyAsync(T.weight, weights, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if (R.classify()) return -1;
    T.built_index = ctx->fleet.stats.built_index;
    Add A{};
    fleet_fill(A, R, weights ? T.weight.get() : nullptr);
    A.c = T.c; A.sums = T.sums;
    A.combine = opt_on(ctx->opt.traffic_combine) ? 1u : 0u;           // (off by default: measured)
    hipLaunchKernelGGL(k_traffic_add, dim3((n + kTrafficBlock - 1) / kTrafficBlock), dim3(kTrafficBlock), 0, ctx->stream, A);
    if (V) hipLaunchKernelGGL(k_traffic_stats, dim3((V + kTrafficBlock - 1) / kTrafficBlock), dim3(kTrafficBlock), 0, ctx->stream, V, T.c.get(), T.vstat.get());
    if (R.finish()) return -1;
    T.ms_kernels = ctx->fleet.stats.ms_kernels;
    if (R.download(code_out, vertex_out, potential_out)) return -1;
  }
  unsigned long long sums[kSums] = {}; uint32_t vstat[kVertexStats] = {};
  HIPCHK(hipMemcpyAsync(sums, T.sums, sizeof(sums), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(vstat, T.vstat, sizeof(vstat), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  T.T += sums[kWeight];
  T.contributing = (uint32_t)sums[kContributing]; T.adds = sums[kAdds];
  T.occupied = vstat[kOccupied]; T.peak = vstat[kPeak];
  T.ms_total = R.ms_total();
  return 0;
}

int mnav_traffic_download(const mnav_ctx* cctx, uint32_t* counts_out)
{
  if (!cctx) return -1;
  mnav_ctx* ctx = const_cast<mnav_ctx*>(cctx);                      // the error string and the stream are the context's
  ctx->err.clear();
  if (!ctx->have_mesh) { ctx->err = "mnav_upload_mesh has not been called"; return -1; }
  if (!counts_out) { ctx->err = "null count array"; return -1; }
  if (!ctx->traffic.c) { memset(counts_out, 0, sizeof(uint32_t) * ctx->V); return 0; }   // no traffic call since the mesh: all zero
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  if (ctx->V) HIPCHK(hipMemcpyAsync(counts_out, ctx->traffic.c, sizeof(uint32_t) * ctx->V, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mnav_traffic_stats(const mnav_ctx* ctx, uint32_t* contributing, uint64_t* adds, uint64_t* total_weight, uint32_t* occupied, uint32_t* peak,
                       uint32_t* built_index, float* ms_kernels, float* ms_total)
{
  if (!ctx) return -1;
  const mnav_traffic::State& T = ctx->traffic;
  if (contributing) *contributing = T.contributing;
  if (adds) *adds = T.adds;
  if (total_weight) *total_weight = T.T;
  if (occupied) *occupied = T.occupied;
  if (peak) *peak = T.peak;
  if (built_index) *built_index = T.built_index;
  if (ms_kernels) *ms_kernels = T.ms_kernels;
  if (ms_total) *ms_total = T.ms_total;
  return 0;
}

// the argument errors of mnav_layer_traffic (and mnav_map_traffic): refused before anything is touched
static int traffic_check_args(mnav_ctx* ctx, double gain, double cap)
{
  if (!ctx->have_mesh) { ctx->err = "mnav_upload_mesh has not been called"; return -1; }
  if (!std::isfinite(gain) || gain < 0.0) { ctx->err = "gain must be finite and >= 0"; return -1; }
  if (std::isnan(cap) || cap < 0.0) { ctx->err = "cap must be >= 0 and not NaN"; return -1; }
  return 0;
}

static int timed_reserve_peak(mnav_ctx* ctx);   // (mnav_timed_capi.h)

// mnav_layer_traffic (timed == false: the rule reads the counts) and mnav_layer_timed_traffic (timed == true: the peaks of
// the timed cells), as they stand
static int traffic_layer_run(mnav_ctx* ctx, bool timed, uint32_t layer, uint32_t free_count, double gain, double cap, uint32_t* changed_out, uint32_t* n_changed)
{
  using namespace mnav_traffic;
  if (!ctx) return -1;
  ctx->err.clear();
  if (traffic_check_args(ctx, gain, cap)) return -1;
  if (layer_slot(ctx, layer, false)) return -1;
  if (timed ? timed_reserve_peak(ctx) : traffic_reserve(ctx, 0)) return -1;
  uint32_t c[mnav_chg::kCounters];
  const TrafficRule rule{ timed ? ctx->timed.peak.get() : ctx->traffic.c.get(), free_count, (float)gain, (float)cap };
  return layer_change_list(ctx, ctx->layers[layer], rule, ctx->ev[7], c, changed_out, n_changed, nullptr);
}

// mnav_map_traffic and mnav_map_timed_traffic: that layer call on an input node of the graph, then the propagation
static int traffic_map_run(mnav_ctx* ctx, bool timed, uint32_t layer, uint32_t free_count, double gain, double cap, uint32_t* changed_out, uint32_t* n_changed)
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
  if (traffic_layer_run(ctx, timed, layer, free_count, gain, cap, nullptr, &nc)) return map_finish(ctx, -1);
  Node& src = S.order[S.pos[layer]];
  src.out = ctx->chg.ids; src.n_out = nc; src.flipped = nc;          // (the slot may have held lethal flags: assume some flipped)
  return map_finish(ctx, map_propagate(ctx, (uint32_t)S.pos[layer], changed_out, n_changed));
}

int mnav_layer_traffic(mnav_ctx* ctx, uint32_t layer, uint32_t free_count, double gain, double cap, uint32_t* changed_out, uint32_t* n_changed)
{
  return traffic_layer_run(ctx, false, layer, free_count, gain, cap, changed_out, n_changed);
}

int mnav_map_traffic(mnav_ctx* ctx, uint32_t layer, uint32_t free_count, double gain, double cap, uint32_t* changed_out, uint32_t* n_changed)
{
  return traffic_map_run(ctx, false, layer, free_count, gain, cap, changed_out, n_changed);
}
