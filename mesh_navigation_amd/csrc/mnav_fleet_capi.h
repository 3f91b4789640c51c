// mnav_fleet_capi.h -- the C ABI of the fleet calls (include/mnav.h: mnav_fleet_paths, mnav_fleet_walks, mnav_fleet_stats)
// over the kernels of mnav_fleet.h, the lookup of mnav_locate_capi.h and k_backtrack.  Included by mnav.hip inside its
// extern "C" block, after mnav_replan_capi.h.
#pragma once

static_assert(mnav_fleet::kSuccess == MNAV_SUCCESS && mnav_fleet::kInvalidStart == MNAV_INVALID_START && mnav_fleet::kInvalidGoal == MNAV_INVALID_GOAL &&
              mnav_fleet::kNoPath == MNAV_NO_PATH_FOUND && mnav_fleet::kInternal == MNAV_INTERNAL_ERROR && mnav_fleet::kBeyond == MNAV_BEYOND_FIELD,
              "mnav_fleet.h restates the codes of include/mnav.h");

constexpr double kFleetScratchMb = 256.0;   // default of the option fleet_scratch_mb

static int fleet_reserve(mnav_ctx* ctx, size_t n, size_t n_slots)
{
  mnav_fleet::State& S = ctx->fleet;
  if (!S.have_ev) {
    for (auto& e : S.ev) HIPCHK(hipEventCreate(e.out()));
    S.have_ev = true;
  }
  if (!S.cnt) HIPCHK(S.cnt.alloc(sizeof(uint32_t) * (mnav_fleet::kCounters + 1)));
  if (n > S.cap) {
    S.cap = 0;
    const size_t nb = (n + mnav_fleet::kFleetBlock - 1) / mnav_fleet::kFleetBlock;
    if (alloc_group(S.slot, 4 * n, S.vtx, 4 * n, S.code, 4 * n, S.len, 4 * n, S.face, 4 * n, S.potential, 4 * n, S.pos, 12 * n, S.status, 4 * n, S.bsum, 8 * nb,
                    S.off, 8 * (n + 1)) != hipSuccess) { ctx->err = "fleet: out of device memory"; return -1; }
    S.cap = n;
  }
  if (n_slots > S.slots_cap) {
    S.slots_cap = 0;
    if (alloc_group(S.fields, sizeof(mnav_fleet::Field) * n_slots, S.wslots, sizeof(mnav_fleet::WalkSlot) * n_slots, S.need, 8 * n_slots) !=
        hipSuccess) {   // (need: a word per plan, then k_fleet_open's answers)
      ctx->err = "fleet: out of device memory"; return -1;
    }
    S.slots_cap = n_slots;
  }
  return 0;
}

// the lookup of n positions for a fleet call: results stay in ctx->loc (q, vtx, face); of the lookup's own statistics only
// `built` may change (the lazy index build is reported as the lookup's, as the follower does)
static int fleet_locate(mnav_ctx* ctx, uint32_t n, const float* pos)
{
  mnav_loc::State& L = ctx->loc;
  const uint32_t built = L.built; const float ms_query = L.ms_query; const uint64_t candidates = L.candidates;
  if (locate_run(ctx, n, pos, 0, nullptr)) return -1;
  ctx->fleet.stats.built_index = L.built;
  if (!L.built) L.built = built;
  L.ms_query = ms_query; L.candidates = candidates;
  return 0;
}

// The statistics of mnav_fleet_stats while another entry point (traffic, timed traffic, schedule) runs the fleet calls'
// shared steps: put back when it ends.
struct FleetStatsKeep {
  mnav_fleet::State& S; const mnav_fleet::Stats kept;
  explicit FleetStatsKeep(mnav_fleet::State& s) : S(s), kept(s.stats) {}
  ~FleetStatsKeep() { S.stats = kept; }
};

// The plans of the recorded Dijkstra call as the robots see them (`who` opens the error text).  Every refusal comes before
// the first device call: a refused call touches nothing.
static int fleet_fields_of(mnav_ctx* ctx, const std::string& who, uint32_t n, const uint32_t* slots, std::vector<mnav_fleet::Field>& fields)
{
  using namespace mnav_fleet;
  if (check_ready(ctx)) return -1;
  if (n > 0x7FFFFFFFu) { ctx->err = who + ": too many robots in one call"; return -1; }
  const Resident& R = ctx->res;
  const size_t n_slots = R.seeds().size();
  if (!R.fields_resident()) {
    ctx->err = who + ": the last plan call was not a Dijkstra call or replan whose fields are resident"; return -1;
  }
  if (ctx->rp.len || ctx->rp.all) { ctx->err = who + ": the costs changed since the plan (mnav_replan_dijkstra_batch first)"; return -1; }
  std::vector<uint8_t> used(n_slots ? n_slots : 1, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (slots[i] >= n_slots) { ctx->err = who + ": slot out of range (not a plan of the last call)"; return -1; }
    used[slots[i]] = 1;
  }
  fields.resize(n_slots);
  for (size_t s = 0; s < n_slots; ++s) {
    Field Fd; Fd.dist = nullptr; Fd.pred = nullptr; Fd.seed = R.seeds()[s]; Fd.target = R.targets()[s]; Fd.cut = INFINITY;
    Fd.code = R.seeds()[s] >= ctx->V ? MNAV_INVALID_START : R.targets()[s] >= ctx->V ? MNAV_INVALID_GOAL : MNAV_SUCCESS;   // what the plan call gave a plan it did not run
    if (used[s] && R.recorded_slot((uint32_t)s) != kNone) {
      // rewindable: "slots[k].dist is the reference's below the cut" (not after the band steps, a failed or cancelled call, a
      // half-rewound replan); on top of it the predecessors must be resident, which a paths-only call does not leave
      Fd.dist = static_cast<const float*>(mnav_device_output(ctx, (uint32_t)s, 0));
      Fd.pred = static_cast<const uint32_t*>(mnav_device_output(ctx, (uint32_t)s, 1));
      if (!R.rewindable() || !Fd.dist || !Fd.pred) {
        ctx->err = who + ": predecessors of slot " + std::to_string(s) + " not resident (a paths-only, band-step, failed or cancelled call)"; return -1;
      }
    }
    fields[s] = Fd;
  }
  return 0;
}

// One fleet call over the robots of the resident fields (paths, plans, traffic, timed traffic, schedule): who asks, the robots
// as the caller gave them, and what the steps leave for the caller's own kernels (P, and d_vtx: where the robots' vertices
// are resident).  begin, classify, the caller's kernels, finish, download.
struct FleetCall {
  mnav_ctx* ctx; const char* who; uint32_t n; const uint32_t* slots; const uint32_t* start_vertex; const float* start_pos;
  std::vector<mnav_fleet::Field> fields; mnav_fleet::Paths P{}; const uint32_t* d_vtx = nullptr;
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();

  // Every refusal comes before the first device call: a refused call touches nothing.  `why`: the caller's own verdict on its
  // position arguments where "a start vertex or a start position" is not its rule (null: they are fine).
  int begin(const char* why)
  {
    if (n && !slots) why = "null slots";
    if (why) { ctx->err = std::string(who) + ": " + why; return -1; }
    return fleet_fields_of(ctx, who, n, slots, fields);
  }
  int begin() { return begin(n && !start_vertex && !start_pos ? "neither start vertices nor start positions" : nullptr); }

  // The robots and the plan records go up, k_fleet_cut and k_fleet_len run (codes, hops, potentials, outcome counters, block
  // sums of the hops); ev[0] is recorded in front of the kernels.
  int classify()
  {
    using namespace mnav_fleet;
    const size_t n_slots = fields.size();
    if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
    if (fleet_reserve(ctx, n, n_slots)) return -1;
    State& S = ctx->fleet;
    S.stats = {};
    d_vtx = S.vtx;
    if (start_vertex) HIPCHK(hipMemcpyAsync(S.vtx, start_vertex, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    else { if (fleet_locate(ctx, n, start_pos)) return -1; d_vtx = ctx->loc.vtx; }   // the ids stay on the device
    HIPCHK(hipMemcpyAsync(S.slot, slots, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(S.fields, fields.data(), sizeof(Field) * n_slots, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(S.cnt, 0, sizeof(uint32_t) * (kCounters + 1), ctx->stream));
    HIPCHK(hipMemsetAsync(S.need, 0, 8 * n_slots, ctx->stream));
    P.n = n; P.V = ctx->V; P.slot = S.slot; P.vtx = d_vtx; P.fields = S.fields; P.code = S.code; P.len = S.len; P.potential = S.potential; P.bsum = S.bsum; P.cnt = S.cnt;
    P.mark = S.status; P.need = S.need;
    const uint32_t nb = (n + kFleetBlock - 1) / kFleetBlock;
    HIPCHK(hipEventRecord(S.ev[0], ctx->stream));
    hipLaunchKernelGGL(k_fleet_cut, dim3(((uint32_t)n_slots + kFleetBlock - 1) / kFleetBlock), dim3(kFleetBlock), 0, ctx->stream, (uint32_t)n_slots, S.fields.get(), ctx->res.offset());
    hipLaunchKernelGGL(k_fleet_len, dim3(nb), dim3(kFleetBlock), 0, ctx->stream, P);
    return 0;
  }

  // After the caller's kernels (with a scan among them: its total): ev[1], the total and the counters come down; robots the
  // wave never reached under a finite cut are settled (did their plans' waves run out?  rule 5) and the statistics' ms_kernels
  // holds the time so far.
  int finish(unsigned long long* total, uint32_t* cnt /* kCounters + 1 */)
  {
    using namespace mnav_fleet;
    State& S = ctx->fleet;
    const uint32_t n_slots = (uint32_t)fields.size(), nb = (n + kFleetBlock - 1) / kFleetBlock;
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.ev[1], ctx->stream));
    HIPCHK(hipMemcpyAsync(total, S.off + n, sizeof(*total), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(cnt, S.cnt, sizeof(uint32_t) * (kCounters + 1), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    S.stats.ms_kernels = ev_ms(S.ev[0], S.ev[1]);
    if (cnt[kCounters]) {
      HIPCHK(hipEventRecord(S.ev[0], ctx->stream));
      hipLaunchKernelGGL(k_fleet_open, dim3(n_slots * kOpenBlocks), dim3(kFleetBlock), 0, ctx->stream, n_slots, ctx->V, S.fields.get(), S.need.get(), S.need + n_slots);
      hipLaunchKernelGGL(k_fleet_resolve, dim3(nb), dim3(kFleetBlock), 0, ctx->stream, P, S.need + n_slots);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(S.ev[1], ctx->stream));
      HIPCHK(hipMemcpyAsync(cnt, S.cnt, sizeof(uint32_t) * (kCounters + 1), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      S.stats.ms_kernels += ev_ms(S.ev[0], S.ev[1]);
    }
    return 0;
  }
  int finish() { unsigned long long unused = 0; uint32_t cnt[mnav_fleet::kCounters + 1] = {}; return finish(&unused, cnt); }   // (no scan ran: the hop total is not this call's)

  // codes, vertices and potentials of the robots, each where the caller wants it: in stream order, no wait
  int download(uint32_t* code_out, uint32_t* vertex_out, float* potential_out)
  {
    if (code_out) HIPCHK(hipMemcpyAsync(code_out, ctx->fleet.code, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (vertex_out) HIPCHK(hipMemcpyAsync(vertex_out, d_vtx, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (potential_out) HIPCHK(hipMemcpyAsync(potential_out, ctx->fleet.potential, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    return 0;
  }

  float ms_total() const { return (float)(1e-3 * (double)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count()); }
  void report(const uint32_t* cnt, unsigned long long total) const    // what mnav_fleet_stats tells of a paths or plans call
  {
    mnav_fleet::Stats& st = ctx->fleet.stats;
    for (int k = 0; k < mnav_fleet::kCounters; ++k) st.outcome[k] = cnt[k];
    st.entries = total; st.ms_total = ms_total();
  }
};

// the robots of a classified call as a kernel's argument record names them (mnav_traffic::Add, mnav_timed::Walk, mnav_schedule::Job)
extern "C++" {
template <class Args>
static void fleet_fill(Args& A, const FleetCall& R, const uint32_t* weight)
{
  A.n = R.P.n; A.V = R.P.V; A.slot = R.P.slot; A.vtx = R.P.vtx; A.fields = R.P.fields; A.code = R.P.code; A.len = R.P.len; A.potential = R.P.potential; A.weight = weight;
}
}  // extern "C++"

int mnav_fleet_paths(mnav_ctx* ctx, uint32_t n, const uint32_t* slots, const uint32_t* start_vertex, const float* start_pos, uint32_t* code_out,
                     uint32_t* vertex_out, float* potential_out, uint32_t* len_out, uint64_t* offset_out, uint32_t* ids_out, uint64_t ids_cap,
                     uint64_t* total_out)
{
  using namespace mnav_fleet;
  if (!ctx) return -1;
  ctx->err.clear();
  if (!n) return 0;
  FleetCall R{ ctx, "fleet paths", n, slots, start_vertex, start_pos };
  if (R.begin() || R.classify()) return -1;
  State& S = ctx->fleet;
  const uint32_t nb = (n + kFleetBlock - 1) / kFleetBlock;
  hipLaunchKernelGGL(k_fleet_scan, dim3(1), dim3(kFleetBlock), 0, ctx->stream, nb, S.bsum.get(), (const unsigned long long*)nullptr, S.off + n);
  hipLaunchKernelGGL(k_fleet_offsets, dim3(nb), dim3(kFleetBlock), 0, ctx->stream, n, S.len.get(), S.bsum.get(), S.off.get());
  unsigned long long total = 0; uint32_t cnt[kCounters + 1] = {};
  if (R.finish(&total, cnt)) return -1;
  const bool fits = ids_out && total <= ids_cap;
  if (fits && total) {
    if (total > S.ids_cap) {
      S.ids_cap = 0;
      if (S.ids.alloc(4 * (size_t)total) != hipSuccess) { ctx->err = "fleet paths: out of device memory"; return -1; }
      S.ids_cap = total;
    }
    HIPCHK(hipEventRecord(S.ev[0], ctx->stream));
    hipLaunchKernelGGL(k_fleet_write, dim3(nb), dim3(kFleetBlock), 0, ctx->stream, R.P, S.off.get(), S.ids.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.ev[1], ctx->stream));
    HIPCHK(hipMemcpyAsync(ids_out, S.ids, 4 * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));   // one dense copy
  }
  if (R.download(code_out, vertex_out, potential_out)) return -1;
  if (len_out) HIPCHK(hipMemcpyAsync(len_out, S.len, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (offset_out) HIPCHK(hipMemcpyAsync(offset_out, S.off, 8 * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (fits && total) S.stats.ms_kernels += ev_ms(S.ev[0], S.ev[1]);
  if (total_out) *total_out = total;
  R.report(cnt, total);
  return fits ? 0 : 1;
}

// buffers of the fleet plans calls: per robot, per plan, per pose of the scratch (ids and lengths), per pose of the output
static int plans_reserve(mnav_ctx* ctx, size_t n, size_t n_plans, unsigned long long scratch, unsigned long long poses)
{
  mnav_fleet::PlanState& PS = ctx->plans;
  const char* oom = "fleet plans: out of device memory";
  if (n > PS.cap) {
    PS.cap = 0;
    if (alloc_group(PS.count, 4 * n, PS.cost, 8 * n) != hipSuccess) { ctx->err = oom; return -1; }
    PS.cap = n;
  }
  if (n_plans > PS.slots_cap) {
    PS.slots_cap = 0;
    if (alloc_group(PS.goal, 12 * n_plans, PS.goal_pose, sizeof(double) * mnav_fleet::kPoseDoubles * n_plans) != hipSuccess) { ctx->err = oom; return -1; }
    PS.slots_cap = n_plans;
  }
  if (scratch > PS.scratch_cap) {
    PS.scratch_cap = 0;
    if (alloc_group(PS.ids, 4 * (size_t)scratch, PS.lengths, 4 * (size_t)scratch) != hipSuccess) { ctx->err = oom; return -1; }
    PS.scratch_cap = scratch;
  }
  if (poses > PS.poses_cap) {
    PS.poses_cap = 0;
    if (PS.poses.alloc(sizeof(double) * mnav_fleet::kPoseDoubles * (size_t)poses) != hipSuccess) { ctx->err = oom; return -1; }
    PS.poses_cap = poses;
  }
  return 0;
}

// mnav_fleet_walks (plans == false: the packed rows go to positions_out / faces_out) and mnav_fleet_walk_plans (plans ==
// true: their poses to poses_out, their costs to cost_out): one walk, two ways out
static int fleet_walks_run(mnav_ctx* ctx, bool plans, uint32_t n, const uint32_t* slots, uint32_t n_plans, const float* seed_pos, const uint32_t* seed_faces,
                           const double* goal_pose, const float* start_pos, const uint32_t* start_faces, double step_width, int32_t inflation_layer,
                           uint32_t walk_cap, int32_t* status_out, uint32_t* start_face_out, uint32_t* len_out, uint64_t* offset_out, float* positions_out,
                           uint32_t* faces_out, double* cost_out, double* poses_out, uint64_t entries_cap, uint64_t* total_out)
{
  using namespace mnav_fleet;
  if (!ctx) return -1;
  ctx->err.clear();
  if (!n) return 0;
  const auto t0 = std::chrono::steady_clock::now();
  // every refusal comes before the first device call: a refused call touches nothing
  if (!slots || !seed_pos || !seed_faces || !start_pos || (plans && !goal_pose)) { ctx->err = "fleet walks: null argument"; return -1; }
  if (!ctx->have_mesh) { ctx->err = "mnav_upload_mesh has not been called"; return -1; }
  if (plans && !ctx->have_face_normals) { ctx->err = "fleet walk plans: face normals are not resident (mnav_upload_face_normals)"; return -1; }
  if (n > 0x7FFFFFFFu) { ctx->err = "fleet walks: too many robots in one call"; return -1; }
  if (walk_cap < 2 || walk_cap > (1u << 24)) { ctx->err = "fleet walks: walk_cap out of range (2 .. 2^24)"; return -1; }
  if (!(step_width > 0.0)) { ctx->err = "step_width must be positive"; return -1; }   // a zero step never leaves the start
  if (n_plans != ctx->res.plans()) { ctx->err = "fleet walks: n_plans differs from the last plan call"; return -1; }
  std::vector<uint8_t> used(n_plans ? n_plans : 1, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (slots[i] >= n_plans) { ctx->err = "fleet walks: slot out of range (not a plan of the last call)"; return -1; }
    if (start_faces && start_faces[i] != kNone && start_faces[i] >= ctx->F) { ctx->err = "fleet walks: face id out of range"; return -1; }
    used[slots[i]] = 1;
  }
  std::vector<WalkSlot> ws(n_plans);
  for (uint32_t s = 0; s < n_plans; ++s) {
    WalkSlot W{};
    W.vecmap = nullptr; W.seed_face = kNone;
    if (used[s] && ctx->res.slot(s) != kNone) {                    // (a plan rejected before it reached the device: status 0, no entries)
      W.vecmap = static_cast<const float*>(mnav_device_output(ctx, s, 4));
      if (!W.vecmap) { ctx->err = "fleet walks: vector map of slot " + std::to_string(s) + " not resident (mnav_set_resident_outputs, or pass vecmap_out to the plan call)"; return -1; }
      if (seed_faces[s] >= ctx->F) { ctx->err = "fleet walks: seed face id out of range"; return -1; }
      W.seed_face = seed_faces[s];
      for (int k = 0; k < 3; ++k) W.seed[k] = seed_pos[3 * (size_t)s + k];
    }
    ws[s] = W;
  }
  WalkInflation L{};
  if (inflation_layer >= 0) {
    if ((size_t)inflation_layer >= ctx->layers.size() || !ctx->layers[inflation_layer].ready || !ctx->layers[inflation_layer].dist || !ctx->layers[inflation_layer].have_vec) {
      ctx->err = "fleet walks: not a resident inflation layer with a vector field"; return -1;
    }
    const mnav_ctx::Layer& Ly = ctx->layers[inflation_layer];
    L.distances = Ly.dist; L.vectors = Ly.vec; L.has_vector = Ly.vstate;
    L.inflation_radius = Ly.inflation_radius; L.inscribed_radius = Ly.inscribed_radius; L.inscribed_value = Ly.inscribed_value; L.lethal_value = Ly.lethal_value;
    L.repulsive_field = 1;
  }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  if (upload_walk_mesh(ctx)) return -1;
  if (fleet_reserve(ctx, n, n_plans)) return -1;
  State& S = ctx->fleet;
  S.stats = {};
  // scratch rows of walk_cap entries (16 bytes each) for one chunk of robots
  const double mb = opt_set(ctx->opt.fleet_scratch_mb) && ctx->opt.fleet_scratch_mb > 0.0 ? ctx->opt.fleet_scratch_mb : kFleetScratchMb;
  const double fit = std::floor(mb * 1048576.0 / (16.0 * (double)walk_cap));
  const uint32_t chunk = (uint32_t)std::min<double>((double)n, std::max(1.0, fit));
  if (chunk > S.rows || walk_cap > S.row_entries) {
    S.rows = S.row_entries = 0;
    if (alloc_group(S.jobs, sizeof(WalkJob) * (size_t)chunk, S.ctl, 8 * (size_t)chunk, S.row_pos, 12 * (size_t)chunk * walk_cap, S.row_face, 4 * (size_t)chunk * walk_cap) !=
        hipSuccess) { ctx->err = "fleet walks: out of device memory"; return -1; }
    S.rows = chunk; S.row_entries = walk_cap;
  }
  const bool want = plans ? poses_out != nullptr : (positions_out || faces_out);
  const unsigned long long out_cap = want ? std::min<unsigned long long>(entries_cap, (unsigned long long)n * walk_cap) : 0ull;
  if (!plans && out_cap > S.out_cap) {
    S.out_cap = 0;
    if (alloc_group(S.out_pos, 12 * (size_t)out_cap, S.out_face, 4 * (size_t)out_cap) != hipSuccess) { ctx->err = "fleet walks: out of device memory"; return -1; }
    S.out_cap = out_cap;
  }
  PlanState& PS = ctx->plans;
  if (plans) {
    if (plans_reserve(ctx, n, n_plans, 0, out_cap)) return -1;
    HIPCHK(hipMemcpyAsync(PS.goal_pose, goal_pose, sizeof(double) * kPoseDoubles * (size_t)n_plans, hipMemcpyHostToDevice, ctx->stream));
  }
  const float* d_pos = S.pos; const uint32_t* d_face = S.face;
  if (start_faces) {
    HIPCHK(hipMemcpyAsync(S.pos, start_pos, 12 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(S.face, start_faces, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  } else { if (fleet_locate(ctx, n, start_pos)) return -1; d_pos = ctx->loc.q; d_face = ctx->loc.face; }   // positions and faces stay on the device
  HIPCHK(hipMemcpyAsync(S.slot, slots, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(S.wslots, ws.data(), sizeof(WalkSlot) * (size_t)n_plans, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(S.cnt, 0, sizeof(uint32_t) * kCounters, ctx->stream));
  const WalkMesh M{ ctx->d_xyz, ctx->d_faces, ctx->d_vf_ptr, ctx->d_vf, ctx->V, ctx->F };
  HIPCHK(hipEventRecord(S.ev[0], ctx->stream));
  for (uint32_t a = 0; a < n; a += chunk) {                           // the chunks follow each other in stream order: one set of scratch rows
    const uint32_t c = std::min(chunk, n - a), nb = (c + kFleetBlock - 1) / kFleetBlock;
    hipLaunchKernelGGL(k_fleet_jobs, dim3(nb), dim3(kFleetBlock), 0, ctx->stream, c, ctx->F, S.slot + a, S.wslots.get(), d_pos + 3 * (size_t)a, d_face + a, S.jobs.get());
    hipLaunchKernelGGL(k_backtrack, dim3(c), dim3(64), 0, ctx->stream, M, L, S.jobs.get(), step_width, walk_cap, S.row_pos.get(), S.row_face.get(), S.ctl.get());
    hipLaunchKernelGGL(k_fleet_walk_len, dim3(nb), dim3(kFleetBlock), 0, ctx->stream, c, ctx->F, d_face + a, S.ctl.get(), S.status + a, S.len + a, S.bsum.get(), S.cnt.get());
    hipLaunchKernelGGL(k_fleet_scan, dim3(1), dim3(kFleetBlock), 0, ctx->stream, nb, S.bsum.get(), a ? S.off + a : (const unsigned long long*)nullptr, S.off + a + c);
    hipLaunchKernelGGL(k_fleet_offsets, dim3(nb), dim3(kFleetBlock), 0, ctx->stream, c, S.len + a, S.bsum.get(), S.off + a);
    if (plans) {                                                      // the rows are robot first already: poses and costs straight from them
      hipLaunchKernelGGL(k_walk_cost, dim3(nb), dim3(kFleetBlock), 0, ctx->stream, c, walk_cap, S.row_pos.get(), S.len + a, PS.cost + a);
      if (out_cap)
        hipLaunchKernelGGL(k_walk_poses, dim3(c), dim3(64), 0, ctx->stream, walk_cap, ctx->F, S.row_pos.get(), S.row_face.get(), S.slot + a, S.len + a, S.off + a,
                           ctx->d_fnrm.get(), PS.goal_pose.get(), PS.poses.get(), out_cap);
    } else if (out_cap)
      hipLaunchKernelGGL(k_fleet_pack, dim3(c), dim3(64), 0, ctx->stream, walk_cap, S.row_pos.get(), S.row_face.get(), S.len + a, S.off + a, S.out_pos.get(), S.out_face.get(), out_cap);
    HIPCHK(hipGetLastError());
    ++S.stats.chunks;
  }
  HIPCHK(hipEventRecord(S.ev[1], ctx->stream));
  unsigned long long total = 0; uint32_t cnt[kCounters] = {};
  HIPCHK(hipMemcpyAsync(&total, S.off + n, sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(cnt, S.cnt, sizeof(cnt), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  S.stats.ms_kernels = ev_ms(S.ev[0], S.ev[1]);
  const bool fits = want && total <= entries_cap;
  if (fits && total && plans) HIPCHK(hipMemcpyAsync(poses_out, PS.poses, sizeof(double) * kPoseDoubles * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
  if (plans && cost_out) HIPCHK(hipMemcpyAsync(cost_out, PS.cost, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (fits && total && !plans) {                                      // two dense copies
    if (positions_out) HIPCHK(hipMemcpyAsync(positions_out, S.out_pos, 12 * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    if (faces_out) HIPCHK(hipMemcpyAsync(faces_out, S.out_face, 4 * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (status_out) HIPCHK(hipMemcpyAsync(status_out, S.status, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (start_face_out) HIPCHK(hipMemcpyAsync(start_face_out, d_face, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (len_out) HIPCHK(hipMemcpyAsync(len_out, S.len, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (offset_out) HIPCHK(hipMemcpyAsync(offset_out, S.off, 8 * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (total_out) *total_out = total;
  for (int k = 0; k < kCounters; ++k) S.stats.outcome[k] = cnt[k];
  S.stats.entries = total;
  S.stats.ms_total = (float)(1e-3 * (double)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count());
  return fits ? 0 : 1;
}

int mnav_fleet_walks(mnav_ctx* ctx, uint32_t n, const uint32_t* slots, uint32_t n_plans, const float* seed_pos, const uint32_t* seed_faces,
                     const float* start_pos, const uint32_t* start_faces, double step_width, int32_t inflation_layer, uint32_t walk_cap,
                     int32_t* status_out, uint32_t* start_face_out, uint32_t* len_out, uint64_t* offset_out, float* positions_out, uint32_t* faces_out,
                     uint64_t entries_cap, uint64_t* total_out)
{
  return fleet_walks_run(ctx, false, n, slots, n_plans, seed_pos, seed_faces, nullptr, start_pos, start_faces, step_width, inflation_layer, walk_cap, status_out,
                         start_face_out, len_out, offset_out, positions_out, faces_out, nullptr, nullptr, entries_cap, total_out);
}

int mnav_fleet_stats(const mnav_ctx* ctx, uint32_t* served, uint32_t* beyond_field, uint32_t* no_path, uint32_t* invalid, uint64_t* entries,
                     uint32_t* built_index, uint32_t* chunks, float* ms_kernels, float* ms_total)
{
  if (!ctx) return -1;
  const mnav_fleet::Stats& S = ctx->fleet.stats;
  if (served) *served = S.outcome[0];
  if (beyond_field) *beyond_field = S.outcome[1];
  if (no_path) *no_path = S.outcome[2];
  if (invalid) *invalid = S.outcome[3];
  if (entries) *entries = S.entries;
  if (built_index) *built_index = S.built_index;
  if (chunks) *chunks = S.chunks;
  if (ms_kernels) *ms_kernels = S.ms_kernels;
  if (ms_total) *ms_total = S.ms_total;
  return 0;
}
