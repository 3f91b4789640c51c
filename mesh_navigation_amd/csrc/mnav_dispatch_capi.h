// mnav_dispatch_capi.h -- the C ABI of fleet dispatch (include/mnav.h: mnav_fleet_costs, mnav_fleet_assign,
// mnav_dispatch_stats) over the kernels of mnav_dispatch.h, k_fleet_cut / k_fleet_open of mnav_fleet.h and the lookup of
// mnav_locate_capi.h.  Included by mnav.hip inside its extern "C" block, after mnav_plans_capi.h.
#pragma once

constexpr double kDispatchMaxMb = 4096.0;              // default of the option dispatch_max_mb
constexpr double kDispatchMaxRounds = 4194304.0;       // default of the option dispatch_max_rounds
constexpr uint32_t kDispatchWideRounds = 32;           // wide rounds per chunk while the mode is wide (4 while it is the tail's)
constexpr uint32_t kDispatchTailRounds = 2048;         // most rounds of one tail launch

// What one matrix pass leaves for its caller: the columns' slot ids, the counters, where the vertices are resident.
struct DispatchRun {
  std::vector<uint32_t> col_slot; unsigned long long cnt[mnav_dispatch::kCounters] = {}; const uint32_t* d_vtx = nullptr;
  uint32_t built_index = 0; float ms_costs = 0.f; bool have_nearest = false;
};

// Every refusal of both calls, before the first device call: a refused call touches nothing.
static int dispatch_check(mnav_ctx* ctx, const std::string& who, uint32_t n, const uint32_t* start_vertex, const float* start_pos, uint32_t m, const uint32_t* slots,
                          double bytes_per_pair, DispatchRun& D, std::vector<mnav_fleet::Field>& cols)
{
  if (!start_vertex && !start_pos) { ctx->err = who + ": neither start vertices nor start positions"; return -1; }
  if (!m) { ctx->err = who + ": no columns"; return -1; }
  if (check_ready(ctx)) return -1;
  std::vector<mnav_fleet::Field> fields;
  if (fleet_fields_of(ctx, who, 0, nullptr, fields)) return -1;             // (the recorded call itself, before anything is said about its slots)
  const size_t n_plans = ctx->res.seeds().size();
  if (!slots && m != n_plans) { ctx->err = who + ": slots == NULL needs m = the plan count of the recorded call"; return -1; }
  D.col_slot.resize(m);
  for (uint32_t j = 0; j < m; ++j) D.col_slot[j] = slots ? slots[j] : j;
  if (fleet_fields_of(ctx, who, m, D.col_slot.data(), fields)) return -1;   // (with its range check of the slots)
  std::vector<uint8_t> seen(fields.size() ? fields.size() : 1, 0);
  for (uint32_t j = 0; j < m; ++j) {
    if (seen[D.col_slot[j]]) { ctx->err = who + ": slot " + std::to_string(D.col_slot[j]) + " given twice"; return -1; }
    seen[D.col_slot[j]] = 1;
  }
  if (n > 0x7FFFFFFFu) { ctx->err = who + ": too many robots in one call"; return -1; }
  const double mb = opt_set(ctx->opt.dispatch_max_mb) && ctx->opt.dispatch_max_mb > 0.0 ? ctx->opt.dispatch_max_mb : kDispatchMaxMb;
  if ((double)n * (double)m * bytes_per_pair > mb * 1048576.0) { ctx->err = who + ": the matrix is larger than dispatch_max_mb"; return -1; }
  cols.resize(m);
  for (uint32_t j = 0; j < m; ++j) cols[j] = fields[D.col_slot[j]];
  return 0;
}

// The matrix pass: codes and potentials of the n x m pairs resident in ctx->dispatch, the counters in D.cnt, the tile minima
// combined when `nearest` is set.
static int dispatch_costs_run(mnav_ctx* ctx, uint32_t n, const uint32_t* start_vertex, const float* start_pos, uint32_t m, const std::vector<mnav_fleet::Field>& cols,
                              bool nearest, DispatchRun& D)
{
  using namespace mnav_dispatch;
  const char* oom = "fleet dispatch: out of device memory";
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  State& S = ctx->dispatch;
  if (!S.have_ev) {
    for (auto& e : S.ev) HIPCHK(hipEventCreate(e.out()));
    S.have_ev = true;
  }
  if (!S.cnt) { if (alloc_group(S.cnt, 8 * kCounters, S.ctl, sizeof(Control), S.info, 8) != hipSuccess) { ctx->err = oom; return -1; } }
  const size_t pairs = (size_t)n * m, RT = (n + kTile - 1) / kTile, CT = (m + kTile - 1) / kTile;
  if (RT * CT > 0x7FFFFFFFull) { ctx->err = "fleet dispatch: too many tiles in one call"; return -1; }
  if (n > S.robots_cap) { S.robots_cap = 0; if (S.vtx.alloc(4 * (size_t)n) != hipSuccess) { ctx->err = oom; return -1; } S.robots_cap = n; }
  if (m > S.cols_cap) {
    S.cols_cap = 0;
    if (alloc_group(S.cols, sizeof(Field) * (size_t)m, S.need, 8 * (size_t)m, S.col_slot, 4 * (size_t)m) != hipSuccess) { ctx->err = oom; return -1; }
    S.cols_cap = m;
  }
  if (pairs > S.pairs_cap) {
    S.pairs_cap = 0;
    if (alloc_group(S.code, pairs, S.potential, 4 * pairs) != hipSuccess) { ctx->err = oom; return -1; }
    S.pairs_cap = pairs;
  }
  if (S.rowpart.bytes() < 8 * CT * n || S.colpart.bytes() < 8 * RT * m) {
    if (alloc_group(S.rowpart, 8 * CT * n, S.colpart, 8 * RT * m) != hipSuccess) { ctx->err = oom; return -1; }
  }
  if ((size_t)n + m > S.nearest_cap) { S.nearest_cap = 0; if (S.nearest.alloc(4 * ((size_t)n + m)) != hipSuccess) { ctx->err = oom; return -1; } S.nearest_cap = (size_t)n + m; }
  D.d_vtx = S.vtx;
  if (start_vertex) HIPCHK(hipMemcpyAsync(S.vtx, start_vertex, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  else {                                                              // the ids stay on the device; of the lookup's statistics only `built` may change
    mnav_loc::State& L = ctx->loc;
    const uint32_t built = L.built; const float ms_query = L.ms_query; const uint64_t candidates = L.candidates;
    if (locate_run(ctx, n, start_pos, 0, nullptr)) return -1;
    D.built_index = L.built;
    if (!L.built) L.built = built;
    L.ms_query = ms_query; L.candidates = candidates;
    D.d_vtx = L.vtx;
  }
  HIPCHK(hipMemcpyAsync(S.cols, cols.data(), sizeof(Field) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(S.col_slot, D.col_slot.data(), 4 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(S.cnt, 0, 8 * kCounters, ctx->stream));
  HIPCHK(hipMemsetAsync(S.need, 0, 8 * (size_t)m, ctx->stream));
  Costs P{};
  P.n = n; P.m = m; P.V = ctx->V; P.vtx = D.d_vtx; P.cols = S.cols; P.code = S.code; P.potential = S.potential; P.rowpart = S.rowpart; P.colpart = S.colpart;
  P.need = S.need; P.cnt = S.cnt;
  HIPCHK(hipEventRecord(S.ev[0], ctx->stream));
  hipLaunchKernelGGL(mnav_fleet::k_fleet_cut, dim3((m + mnav_fleet::kFleetBlock - 1) / mnav_fleet::kFleetBlock), dim3(mnav_fleet::kFleetBlock), 0, ctx->stream, m, S.cols.get(),
                     ctx->res.offset());
  hipLaunchKernelGGL(k_dispatch_costs, dim3((uint32_t)(RT * CT)), dim3(kDispBlock), 0, ctx->stream, P);
  if (nearest) hipLaunchKernelGGL(k_dispatch_nearest, dim3((n + m + kDispBlock - 1) / kDispBlock), dim3(kDispBlock), 0, ctx->stream, n, m, S.rowpart.get(), S.colpart.get(), S.nearest.get(), S.nearest + n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(S.ev[1], ctx->stream));
  HIPCHK(hipMemcpyAsync(D.cnt, S.cnt, 8 * kCounters, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  D.ms_costs = ev_ms(S.ev[0], S.ev[1]);
  if (D.cnt[5]) {                                                     // rule 5 under a finite cut: did the marked columns' waves run out?
    const uint32_t blocks = (uint32_t)std::min<size_t>((pairs + kDispBlock - 1) / kDispBlock, 65536);
    HIPCHK(hipEventRecord(S.ev[0], ctx->stream));
    hipLaunchKernelGGL(mnav_fleet::k_fleet_open, dim3(m * mnav_fleet::kOpenBlocks), dim3(mnav_fleet::kFleetBlock), 0, ctx->stream, m, ctx->V, S.cols.get(), S.need.get(), S.need + m);
    hipLaunchKernelGGL(k_dispatch_resolve, dim3(blocks), dim3(kDispBlock), 0, ctx->stream, (unsigned long long)pairs, m, S.code.get(), S.need + m, S.cnt.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.ev[1], ctx->stream));
    HIPCHK(hipMemcpyAsync(D.cnt, S.cnt, 8 * kCounters, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    D.ms_costs += ev_ms(S.ev[0], S.ev[1]);
  }
  D.have_nearest = nearest;
  return 0;
}

static float dispatch_ms_since(std::chrono::steady_clock::time_point t0)
{
  return (float)(1e-3 * (double)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count());
}

int mnav_fleet_costs(mnav_ctx* ctx, uint32_t n, const uint32_t* start_vertex, const float* start_pos, uint32_t m, const uint32_t* slots, uint8_t* code_out,
                     float* potential_out, uint32_t* vertex_out, uint32_t* nearest_slot_out, uint32_t* nearest_robot_out)
{
  using namespace mnav_dispatch;
  if (!ctx) return -1;
  ctx->err.clear();
  if (!n) return 0;
  const auto t0 = std::chrono::steady_clock::now();
  DispatchRun D; std::vector<Field> cols;
  if (dispatch_check(ctx, "fleet costs", n, start_vertex, start_pos, m, slots, 5.0, D, cols)) return -1;
  if (dispatch_costs_run(ctx, n, start_vertex, start_pos, m, cols, true, D)) return -1;
  State& S = ctx->dispatch;
  const size_t pairs = (size_t)n * m;
  if (code_out) HIPCHK(hipMemcpyAsync(code_out, S.code, pairs, hipMemcpyDeviceToHost, ctx->stream));
  if (potential_out) HIPCHK(hipMemcpyAsync(potential_out, S.potential, 4 * pairs, hipMemcpyDeviceToHost, ctx->stream));
  if (vertex_out) HIPCHK(hipMemcpyAsync(vertex_out, D.d_vtx, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (nearest_slot_out) HIPCHK(hipMemcpyAsync(nearest_slot_out, S.nearest, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (nearest_robot_out) HIPCHK(hipMemcpyAsync(nearest_robot_out, S.nearest + n, 4 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  Stats T;
  for (int k = 0; k < 4; ++k) T.pairs[k] = D.cnt[k];
  T.feasible = D.cnt[4]; T.built_index = D.built_index; T.ms_costs = D.ms_costs;
  T.ms_total = dispatch_ms_since(t0);
  S.stats = T;
  return 0;
}

int mnav_fleet_assign(mnav_ctx* ctx, uint32_t n, const uint32_t* start_vertex, const float* start_pos, uint32_t m, const uint32_t* slots, double quantum,
                      uint32_t* slot_of_robot_out, uint32_t* robot_of_slot_out, float* potential_out, uint32_t* assigned_out, int64_t* total_q_out,
                      double* total_potential_out)
{
  using namespace mnav_dispatch;
  if (!ctx) return -1;
  ctx->err.clear();
  if (!n) return 0;
  const auto t0 = std::chrono::steady_clock::now();
  const char* oom = "fleet assign: out of device memory";
  if (!(quantum > 0.0) || !std::isfinite(quantum)) { ctx->err = "fleet assign: the quantum must be finite and positive"; return -1; }
  DispatchRun D; std::vector<Field> cols;
  if (dispatch_check(ctx, "fleet assign", n, start_vertex, start_pos, m, slots, 9.0, D, cols)) return -1;
  if (dispatch_costs_run(ctx, n, start_vertex, start_pos, m, cols, false, D)) return -1;
  State& S = ctx->dispatch;
  const size_t pairs = (size_t)n * m;
  const uint32_t N = n > m ? n : m;
  if (pairs > S.q_cap) { S.q_cap = 0; if (S.q.alloc(4 * pairs) != hipSuccess) { ctx->err = oom; return -1; } S.q_cap = pairs; }
  if (N > S.auction_cap) {
    S.auction_cap = 0;
    if (alloc_group(S.price, 8 * (size_t)N, S.bidval, 8 * (size_t)N, S.colbest, 8 * (size_t)N, S.words, 16 * (size_t)N) != hipSuccess) { ctx->err = oom; return -1; }
    S.auction_cap = N;
  }
  if (n > S.result_cap) { S.result_cap = 0; if (S.result.alloc(16 * (size_t)n) != hipSuccess) { ctx->err = oom; return -1; } S.result_cap = n; }
  // quantise once
  uint32_t info[2] = { 0, 0 };
  HIPCHK(hipEventRecord(S.ev[0], ctx->stream));
  HIPCHK(hipMemsetAsync(S.info, 0, 8, ctx->stream));
  hipLaunchKernelGGL(k_dispatch_quantise, dim3((uint32_t)std::min<size_t>((pairs + kDispBlock - 1) / kDispBlock, 65536)), dim3(kDispBlock), 0, ctx->stream, (unsigned long long)pairs,
                     S.code.get(), S.potential.get(), quantum, S.q.get(), S.info.get());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(info, S.info, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (info[1]) { ctx->err = "fleet assign: a quantised cost above 2^31 - 1 (quantum too fine)"; return -1; }
  const long long qmax = info[0];
  const unsigned __int128 top = (unsigned __int128)((unsigned long long)N + 1) * ((unsigned __int128)N * (unsigned long long)qmax + 1);
  if (top >= ((unsigned __int128)1 << 56)) { ctx->err = "fleet assign: quantum too fine for this fleet"; return -1; }
  Auction A{};
  A.n = n; A.m = m; A.N = N;
  const uint32_t tail = opt_u32(ctx->opt.dispatch_tail_bidders, kTailDefault);
  A.tail = tail < kTailMax ? tail : kTailMax;
  A.q = S.q; A.scale = (long long)N + 1; A.big = ((long long)N * qmax + 1) * A.scale;
  const double cap = opt_set(ctx->opt.dispatch_max_rounds) && ctx->opt.dispatch_max_rounds >= 1.0 ? ctx->opt.dispatch_max_rounds : kDispatchMaxRounds;
  A.max_rounds = (unsigned long long)cap;
  A.price = S.price; A.bidval = S.bidval; A.colbest = S.colbest;
  A.owner = S.words; A.mine = S.words + N; A.bidcol = S.words + 2 * (size_t)N; A.winner = S.words + 3 * (size_t)N;
  A.ctl = S.ctl;
  const long long C = D.cnt[4] < (unsigned long long)pairs ? A.big : qmax * A.scale;   // the largest scaled cost
  Control c{};
  c.eps = C / 2 > 1 ? C / 2 : 1; c.unassigned = N; c.phases = 1; c.mode = N <= A.tail ? kModeTail : kModeWide;
  HIPCHK(hipMemsetAsync(S.price, 0, 8 * (size_t)N, ctx->stream));
  HIPCHK(hipMemsetAsync(S.colbest, 0, 8 * (size_t)N, ctx->stream));
  HIPCHK(hipMemsetAsync(S.words, 0xFF, 16 * (size_t)N, ctx->stream));
  HIPCHK(hipMemcpyAsync(S.ctl, &c, sizeof(c), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));                          // (c is on the stack)
  const uint32_t tail_budget = (uint32_t)std::max<unsigned long long>(16ull, std::min<unsigned long long>(kDispatchTailRounds, (1ull << 28) / ((unsigned long long)std::max(1u, A.tail) * N)));
  while (!c.flags) {
    const uint32_t wide = c.mode == kModeWide ? kDispatchWideRounds : 4u;
    if (c.mode == kModeTail) hipLaunchKernelGGL(k_dispatch_tail, dim3(1), dim3(kAuctionBlock), 0, ctx->stream, A, tail_budget);
    for (uint32_t r = 0; r < wide; ++r) {
      hipLaunchKernelGGL(k_dispatch_bid, dim3((N + kDispBlock / 64 - 1) / (kDispBlock / 64)), dim3(kDispBlock), 0, ctx->stream, A);
      hipLaunchKernelGGL(k_dispatch_award, dim3(1), dim3(kAuctionBlock), 0, ctx->stream, A);
    }
    if (c.mode == kModeWide && A.tail) hipLaunchKernelGGL(k_dispatch_tail, dim3(1), dim3(kAuctionBlock), 0, ctx->stream, A, tail_budget);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&c, S.ctl, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  if (c.flags & kFlagOverflow) { ctx->err = "fleet assign: a bid reached 2^62"; return -1; }
  if (!(c.flags & kFlagDone)) { ctx->err = "fleet assign: dispatch_max_rounds reached after " + std::to_string(c.rounds) + " rounds"; return -1; }
  uint32_t* r_col = S.result; uint32_t* r_slot = S.result + n; float* r_pot = reinterpret_cast<float*>(S.result + 2 * (size_t)n);
  int32_t* r_q = reinterpret_cast<int32_t*>(S.result + 3 * (size_t)n);
  hipLaunchKernelGGL(k_dispatch_result, dim3((n + kDispBlock - 1) / kDispBlock), dim3(kDispBlock), 0, ctx->stream, A, S.potential.get(), S.col_slot.get(), r_col, r_slot, r_pot, r_q);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(S.ev[1], ctx->stream));
  std::vector<uint32_t> host(4 * (size_t)n);
  HIPCHK(hipMemcpyAsync(host.data(), S.result, 16 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  // only n-sized arrays came down: the sums in robot order, the columns' robots
  uint32_t assigned = 0; long long total_q = 0; double total_pot = 0.0;
  if (robot_of_slot_out) for (uint32_t j = 0; j < m; ++j) robot_of_slot_out[j] = MNAV_NONE;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t j = host[i];
    float pot; memcpy(&pot, &host[2 * (size_t)n + i], 4);
    if (j != MNAV_NONE) {
      ++assigned; total_q += (int32_t)host[3 * (size_t)n + i]; total_pot += (double)pot;
      if (robot_of_slot_out) robot_of_slot_out[j] = i;
    }
    if (slot_of_robot_out) slot_of_robot_out[i] = host[(size_t)n + i];
    if (potential_out) potential_out[i] = pot;
  }
  if (assigned_out) *assigned_out = assigned;
  if (total_q_out) *total_q_out = total_q;
  if (total_potential_out) *total_potential_out = total_pot;
  Stats T;
  for (int k = 0; k < 4; ++k) T.pairs[k] = D.cnt[k];
  T.feasible = D.cnt[4]; T.built_index = D.built_index; T.ms_costs = D.ms_costs;
  T.assigned = assigned; T.phases = c.phases; T.rounds = c.rounds; T.tail_rounds = c.tail_rounds; T.bids = c.bids;
  T.ms_assign = ev_ms(S.ev[0], S.ev[1]);
  T.ms_total = dispatch_ms_since(t0);
  S.stats = T;
  return 0;
}

int mnav_dispatch_stats(const mnav_ctx* ctx, uint64_t* pairs, uint64_t* feasible, uint32_t* assigned, uint32_t* phases, uint64_t* rounds, uint64_t* tail_rounds,
                        uint64_t* bids, uint32_t* built_index, float* ms_costs, float* ms_assign, float* ms_total)
{
  if (!ctx) return -1;
  const mnav_dispatch::Stats& T = ctx->dispatch.stats;
  if (pairs) for (int k = 0; k < 4; ++k) pairs[k] = T.pairs[k];
  if (feasible) *feasible = T.feasible;
  if (assigned) *assigned = T.assigned;
  if (phases) *phases = T.phases;
  if (rounds) *rounds = T.rounds;
  if (tail_rounds) *tail_rounds = T.tail_rounds;
  if (bids) *bids = T.bids;
  if (built_index) *built_index = T.built_index;
  if (ms_costs) *ms_costs = T.ms_costs;
  if (ms_assign) *ms_assign = T.ms_assign;
  if (ms_total) *ms_total = T.ms_total;
  return 0;
}
