// mnav_schedule_capi.h -- the C ABI of the fleet schedule (include/mnav.h: mnav_fleet_schedule, mnav_schedule_stats) over
// the kernels of mnav_schedule.h, the TimedCells and the peak pass of mnav_timed_capi.h and the FleetCall of
// mnav_fleet_capi.h.  Included by mnav.hip inside its extern "C" block, after mnav_timed_capi.h.
#pragma once

static_assert(mnav_schedule::kStNone == MNAV_SCHEDULE_NONE && mnav_schedule::kStCommitted == MNAV_SCHEDULE_COMMITTED &&
              mnav_schedule::kStNoSlot == MNAV_SCHEDULE_NO_SLOT && mnav_schedule::kStOpen == MNAV_SCHEDULE_OPEN &&
              mnav_schedule::kSeedFree == MNAV_SCHEDULE_SEED_FREE, "mnav_schedule.h restates the values of include/mnav.h");

// the tentative arrays of `cells` cells (clean), the control record and room for n robots
static int schedule_reserve(mnav_ctx* ctx, size_t n, size_t cells)
{
  using namespace mnav_schedule;
  State& S = ctx->schedule;
  const char* oom = "fleet schedule: out of device memory";
  if (!S.ctl && S.ctl.alloc(sizeof(Counts)) != hipSuccess) { ctx->err = oom; return -1; }
  if (cells != S.cells || !S.tent) {
    S.cells = 0;
    if (alloc_group(S.tent, 4 * cells, S.thold, 8 * cells) != hipSuccess) { ctx->err = oom; return -1; }
    S.cells = cells; S.dirty = true;
  }
  if (S.dirty) {
    HIPCHK(hipMemsetAsync(S.tent, 0, 4 * cells, ctx->stream));
    HIPCHK(hipMemsetAsync(S.thold, 0xFF, 8 * cells, ctx->stream));
    S.dirty = false;
  }
  if (n > S.cap) {
    S.cap = 0;
    if (alloc_group(S.list, 8 * n, S.st, 4 * n, S.cur, 4 * n, S.win, 4 * n, S.delay, 4 * n, S.round, 4 * n, S.depart_out, 4 * n) != hipSuccess) { ctx->err = oom; return -1; }
    S.cap = n;
  }
  return 0;
}

int mnav_fleet_schedule(mnav_ctx* ctx, uint32_t n, const uint32_t* slots, const uint32_t* start_vertex, const float* start_pos, const uint32_t* weights,
                        const float* depart, const float* pace, const uint32_t* key, uint32_t windows, double tau, uint32_t capacity, uint32_t max_delay,
                        uint32_t max_rounds, uint32_t flags, int accumulate, uint32_t* code_out, uint32_t* vertex_out, float* potential_out,
                        uint32_t* status_out, uint32_t* delay_out, float* depart_out, uint32_t* round_out)
{
  using namespace mnav_schedule;
  if (!ctx) return -1;
  ctx->err.clear();
  if (!n && accumulate) return 0;                                     // (n = 0 without `accumulate` still starts the cells over)
  FleetCall R{ ctx, "fleet schedule", n, slots, start_vertex, start_pos };
  if (R.begin()) return -1;
  mnav_timed::State& T = ctx->timed;
  State& S = ctx->schedule;
  TimedCells C{ ctx, n, windows, tau, accumulate };
  const uint32_t B = windows;
  const char* why = mnav_timed::timed_refusal(n, weights, depart, pace, B, tau, accumulate, T.T, T.cell ? T.B : 0u, T.tau);
  if (!why) why = schedule_refusal(B, capacity, max_delay, flags);
  if (why) { ctx->err = std::string("fleet schedule: ") + why; return -1; }
  if (C.too_large((double)kBytesPerCell, "fleet schedule: cells, holders and the tentative arrays are larger than timed_traffic_max_mb")) return -1;
  FleetStatsKeep keep(ctx->fleet);
  const size_t cells = C.cells();
  if (C.reserve() || schedule_reserve(ctx, n, cells) || C.reset()) return -1;   // (the tentative arrays before the cells start over)
  HIPCHK(hipMemsetAsync(S.ctl, 0, sizeof(Counts), ctx->stream));
  S.last = Counts{}; S.built_index = 0; S.ms_kernels = 0.f;
  mnav_fleet::State& FS = ctx->fleet;
  Counts K = {};
  if (n) {
    if (C.upload(weights, depart, pace, key) || R.classify()) return -1;
    S.built_index = T.built_index = FS.stats.built_index;
    const uint32_t rounds_most = max_rounds ? std::min(max_rounds, n) : n;   // progress: a round commits a robot or ends the loop
    const uint32_t chunk = std::max(1u, opt_u32(ctx->opt.schedule_chunk_rounds, kChunkRounds));
    const bool fill = opt_on(ctx->opt.schedule_clean_fill);
    Job J{};
    timed_fill(J, C, R);
    J.capacity = capacity; J.max_delay = max_delay; J.limit = rounds_most; J.flags = flags; J.undo = fill ? 0u : 1u;
    J.tent = S.tent; J.thold = S.thold; J.ctl = S.ctl; J.list = S.list;
    J.st = S.st; J.cur = S.cur; J.win = S.win; J.delay_out = S.delay; J.round_out = S.round; J.depart_out = S.depart_out;
    const dim3 lanes((n + kScheduleBlock - 1) / kScheduleBlock), waves((n + kScheduleBlock / 64 - 1) / (kScheduleBlock / 64)), block(kScheduleBlock);
    // `chunk` rounds in stream order; the kernels of a round that has nothing to do return at once
    auto enqueue = [&](uint32_t rounds, bool first) {
      for (uint32_t r = 0; r < rounds; ++r) {
        if (fill && !(first && r == 0)) {
          if (hipMemsetAsync(S.tent, 0, 4 * cells, ctx->stream) != hipSuccess || hipMemsetAsync(S.thold, 0xFF, 8 * cells, ctx->stream) != hipSuccess) return -1;
        }
        hipLaunchKernelGGL(k_schedule_probe, waves, block, 0, ctx->stream, J);
        hipLaunchKernelGGL(k_schedule_claim, lanes, block, 0, ctx->stream, J);
        hipLaunchKernelGGL(k_schedule_decide, lanes, block, 0, ctx->stream, J);
        hipLaunchKernelGGL(k_schedule_commit, lanes, block, 0, ctx->stream, J);
        hipLaunchKernelGGL(k_schedule_next, dim3(1), dim3(1), 0, ctx->stream, J);
      }
      return 0;
    };
    if (fill) S.dirty = true;
    // the host loop's bound does not depend on device data: the first chunk rides on the classification's own look
    const uint32_t chunks_most = (rounds_most + chunk - 1) / chunk + 1u;
    hipLaunchKernelGGL(k_schedule_init, lanes, block, 0, ctx->stream, J);
    if (enqueue(std::min(chunk, rounds_most), true)) { ctx->err = "fleet schedule: hipMemsetAsync failed"; return -1; }
    HIPCHK(hipMemcpyAsync(&K, S.ctl, sizeof(K), hipMemcpyDeviceToHost, ctx->stream));
    if (R.finish()) return -1;                                        // synchronises: K is the record after the first chunk
    S.ms_kernels = FS.stats.ms_kernels;
    for (uint32_t c = 1; c < chunks_most && K.open && K.round < rounds_most; ++c) {
      HIPCHK(hipEventRecord(FS.ev[0], ctx->stream));
      if (enqueue(std::min(chunk, rounds_most - K.round), false)) { ctx->err = "fleet schedule: hipMemsetAsync failed"; return -1; }
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(FS.ev[1], ctx->stream));
      HIPCHK(hipMemcpyAsync(&K, S.ctl, sizeof(K), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      S.ms_kernels += ev_ms(FS.ev[0], FS.ev[1]);
    }
    HIPCHK(hipEventRecord(FS.ev[0], ctx->stream));
    if (timed_peak(ctx, B, capacity)) return -1;
    HIPCHK(hipEventRecord(FS.ev[1], ctx->stream));
    if (R.download(code_out, vertex_out, potential_out)) return -1;
    if (status_out) HIPCHK(hipMemcpyAsync(status_out, S.st, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (delay_out) HIPCHK(hipMemcpyAsync(delay_out, S.delay, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (depart_out) HIPCHK(hipMemcpyAsync(depart_out, S.depart_out, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (round_out) HIPCHK(hipMemcpyAsync(round_out, S.round, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  } else if (timed_peak(ctx, B, capacity)) return -1;
  if (C.read_words()) return -1;
  if (n) S.ms_kernels += ev_ms(FS.ev[0], FS.ev[1]);
  // the cells as if the committed robots had been a timed call's contributors
  T.T += K.weight;
  T.contributing = K.committed; T.adds = K.visits; T.beyond = 0;
  T.yielding = 0; T.ms_kernels = S.ms_kernels;
  S.last = K;
  S.ms_total = T.ms_total = R.ms_total();
  return 0;
}

int mnav_schedule_stats(const mnav_ctx* ctx, uint32_t* contributing, uint32_t* committed, uint32_t* no_slot, uint32_t* open, uint32_t* rounds, uint32_t* delayed,
                        uint32_t* max_delay_used, uint64_t* claims, uint64_t* committed_visits, uint32_t* built_index, float* ms_kernels, float* ms_total)
{
  if (!ctx) return -1;
  const mnav_schedule::State& S = ctx->schedule;
  if (contributing) *contributing = S.last.contributing;
  if (committed) *committed = S.last.committed;
  if (no_slot) *no_slot = S.last.no_slot;
  if (open) *open = S.last.open;
  if (rounds) *rounds = S.last.round;
  if (delayed) *delayed = S.last.delayed;
  if (max_delay_used) *max_delay_used = S.last.max_delay_used;
  if (claims) *claims = S.last.claims;
  if (committed_visits) *committed_visits = S.last.visits;
  if (built_index) *built_index = S.built_index;
  if (ms_kernels) *ms_kernels = S.ms_kernels;
  if (ms_total) *ms_total = S.ms_total;
  return 0;
}
