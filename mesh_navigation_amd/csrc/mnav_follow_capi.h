// mnav_follow_capi.h -- the C ABI of the vector-field follower (include/mnav.h: mnav_follow_batch, mnav_follow_stats)
// over the kernels of mnav_follow.h.  Included by mnav.hip inside its extern "C" block, after mnav_locate_capi.h (the
// lazy index build is the lookup's own).
#pragma once

static_assert(sizeof(mnav_follow_config) == sizeof(mnav_fol::Config) && offsetof(mnav_follow_config, max_search_distance) == offsetof(mnav_fol::Config, max_search_distance),
              "mnav_follow_config and mnav_fol::Config are one layout");

// The argument checks of a follower call (mnav_follow_batch, mnav_follow_rollout), all on the host: -1 with ctx->err set, or
// 0 and maps[s] = the resident vector map of every slot a robot uses (null for the others).
static int follow_check(mnav_ctx* ctx, uint32_t n, const float* pos, const float* dir, const float* up, const uint32_t* face_in, const uint32_t* slots,
                        const uint32_t* seed_faces, const mnav_follow_config* config, std::vector<const float*>& maps)
{
  using mnav_fol::kNone;
  if (!pos || !dir || !up || !face_in || !slots || !config) { ctx->err = "follow: null argument"; return -1; }
  if (check_ready(ctx)) return -1;
  if (n > 0x7FFFFFFFu) { ctx->err = "follow: too many robots in one call"; return -1; }
  if (!(config->max_search_radius > 0.0) || !std::isfinite(config->max_search_radius)) { ctx->err = "follow: max_search_radius must be positive and finite"; return -1; }
  if (!(config->max_search_distance > 0.0) || !std::isfinite(config->max_search_distance)) { ctx->err = "follow: max_search_distance must be positive and finite"; return -1; }
  const size_t n_slots = ctx->res.plans();
  maps.assign(n_slots ? n_slots : 1, nullptr);
  std::vector<uint8_t> used(n_slots ? n_slots : 1, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (slots[i] >= n_slots) { ctx->err = "follow: slot out of range (not a plan of the last call)"; return -1; }
    if (face_in[i] != kNone && face_in[i] >= ctx->F) { ctx->err = "follow: face id out of range"; return -1; }
    if (seed_faces && seed_faces[i] != kNone && seed_faces[i] >= ctx->F) { ctx->err = "follow: seed face id out of range"; return -1; }
    used[slots[i]] = 1;
  }
  for (size_t s = 0; s < n_slots; ++s) {
    if (!used[s]) continue;
    maps[s] = static_cast<const float*>(mnav_device_output(ctx, (uint32_t)s, 4));
    if (!maps[s]) { ctx->err = "follow: vector map of slot " + std::to_string(s) + " not resident (mnav_set_resident_outputs, or pass vecmap_out to the plan call)"; return -1; }
  }
  return 0;
}

// the context's staging for n robots over n_slots plans (mnav_fol::Staging); `what`: the caller's name in the refusal
static int staging_reserve(mnav_ctx* ctx, size_t n, size_t n_slots, const char* what)
{
  mnav_fol::Staging& G = ctx->stage;
  if (!G.have_ev) {
    for (auto& e : G.ev) HIPCHK(hipEventCreate(e.out()));
    G.have_ev = true;
  }
  if (n > G.cap) {
    G.cap = 0;
    if (alloc_group(G.pos, 12 * n, G.dir, 12 * n, G.up, 12 * n, G.face, 4 * n, G.slot, 4 * n, G.seed_face, 4 * n, G.nb_list, 4 * n, G.gl_list, 4 * n) !=
        hipSuccess) { ctx->err = std::string(what) + ": out of device memory"; return -1; }
    G.cap = n;
  }
  if (n_slots > G.slots_cap) {
    G.slots_cap = 0;
    HIPCHK(G.vecmaps.alloc(sizeof(const float*) * n_slots));
    G.slots_cap = n_slots;
  }
  return 0;
}

// every input of a call into the staging (on the context's stream), and the part of the passes' view that points into it
static int staging_upload(mnav_ctx* ctx, uint32_t n, const float* pos, const float* dir, const float* up, const uint32_t* face_in, const uint32_t* slots,
                          const uint32_t* seed_faces, const std::vector<const float*>& maps, mnav_fol::Robots& R)
{
  mnav_fol::Staging& G = ctx->stage;
  HIPCHK(hipMemcpyAsync(G.pos, pos, 12 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(G.dir, dir, 12 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(G.up, up, 12 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(G.face, face_in, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(G.slot, slots, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  if (seed_faces) HIPCHK(hipMemcpyAsync(G.seed_face, seed_faces, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(G.vecmaps, maps.data(), sizeof(const float*) * ctx->res.plans(), hipMemcpyHostToDevice, ctx->stream));
  R.n = n; R.slot = G.slot; R.seed_face = seed_faces ? G.seed_face.get() : nullptr; R.vecmaps = G.vecmaps; R.costs = ctx->d_cost;
  R.nb_list = G.nb_list; R.gl_list = G.gl_list;
  return 0;
}

static int follow_reserve(mnav_ctx* ctx, size_t n)
{
  mnav_fol::State& S = ctx->fol;
  if (!S.cnt) HIPCHK(S.cnt.alloc(sizeof(uint32_t) * mnav_fol::kCounters));
  if (n > S.cap) {
    S.cap = 0;
    if (alloc_group(S.code, 4 * n, S.face, 4 * n, S.bary, 12 * n, S.pos_out, 12 * n, S.mesh_dir, 12 * n, S.cost, 4 * n, S.cmd, 16 * n, S.how, 4 * n) !=
        hipSuccess) { ctx->err = "follow: out of device memory"; return -1; }
    S.cap = n;
  }
  return 0;
}

int mnav_follow_batch(mnav_ctx* ctx, uint32_t n, const float* pos, const float* dir, const float* up, const uint32_t* face_in, const uint32_t* slots,
                      const uint32_t* seed_faces, const mnav_follow_config* config, int32_t* code_out, uint32_t* face_out, float* bary_out,
                      float* pos_out, float* mesh_dir_out, float* cost_out, double* cmd_out, int32_t* how_out)
{
  using namespace mnav_fol;
  if (!ctx) return -1;
  ctx->err.clear();
  if (!n) return 0;
  const auto t0 = std::chrono::steady_clock::now();
  // every refusal comes before the first device call: a refused call touches nothing
  std::vector<const float*> maps;
  if (follow_check(ctx, n, pos, dir, up, face_in, slots, seed_faces, config, maps)) return -1;
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  if (upload_walk_mesh(ctx)) return -1;
  if (staging_reserve(ctx, n, ctx->res.plans(), "follow") || follow_reserve(ctx, n)) return -1;
  State& S = ctx->fol;
  Staging& G = ctx->stage;
  S.stayed = S.neighbour = S.global = S.lost = S.no_field = S.built_index = 0; S.ms_kernels = S.ms_total = 0.f;
  Batch B{};
  if (staging_upload(ctx, n, pos, dir, up, face_in, slots, seed_faces, maps, B)) return -1;
  HIPCHK(hipMemsetAsync(S.cnt, 0, sizeof(uint32_t) * kCounters, ctx->stream));
  B.pos = G.pos; B.dir = G.dir; B.up = G.up; B.face_in = G.face; B.cnt = S.cnt;
  B.code = S.code; B.face = S.face; B.bary = S.bary; B.pos_out = S.pos_out; B.mesh_dir = S.mesh_dir; B.cost = S.cost; B.cmd = S.cmd; B.how = S.how;
  Config C;
  std::memcpy(&C, config, sizeof(C));
  const WalkMesh M{ ctx->d_xyz, ctx->d_faces, ctx->d_vf_ptr, ctx->d_vf, ctx->V, ctx->F };
  HIPCHK(hipEventRecord(G.ev[0], ctx->stream));
  hipLaunchKernelGGL(k_follow_stay, dim3((n + kStayBlock - 1) / kStayBlock), dim3(kStayBlock), 0, ctx->stream, B, M, C);
  hipLaunchKernelGGL(k_follow_search, dim3(n < 2048u ? n : 2048u), dim3(64), 0, ctx->stream, B, M, C);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(G.ev[1], ctx->stream));
  uint32_t cnt[kCounters] = {};
  HIPCHK(hipMemcpyAsync(cnt, S.cnt, sizeof(cnt), hipMemcpyDeviceToHost, ctx->stream));   // the one look at the list lengths
  HIPCHK(hipStreamSynchronize(ctx->stream));
  S.ms_kernels = ev_ms(G.ev[0], G.ev[1]);
  const uint32_t n_gl = cnt[1];
  if (n_gl > n) { ctx->err = "follow: work list out of range"; return -1; }
  if (n_gl) {
    if (locate_ensure(ctx, &S.built_index)) return -1;                // the index mnav_locate would build, and reports as its own
    const mnav_loc::State& L = ctx->loc;
    const mnav_loc::Index I{ L.nodes, L.pts, L.n_pts, L.n_leaves, mnav_loc::loc_root(L.n_leaves) };
    HIPCHK(hipEventRecord(G.ev[2], ctx->stream));
    hipLaunchKernelGGL(k_follow_global, dim3((n_gl + mnav_loc::kLocBlock - 1) / mnav_loc::kLocBlock), dim3(mnav_loc::kLocBlock), 0, ctx->stream, B, M, C, I,
                       n_gl);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(G.ev[3], ctx->stream));
    HIPCHK(hipMemcpyAsync(cnt, S.cnt, sizeof(cnt), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (code_out) HIPCHK(hipMemcpyAsync(code_out, S.code, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (face_out) HIPCHK(hipMemcpyAsync(face_out, S.face, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (bary_out) HIPCHK(hipMemcpyAsync(bary_out, S.bary, 12 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (pos_out) HIPCHK(hipMemcpyAsync(pos_out, S.pos_out, 12 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (mesh_dir_out) HIPCHK(hipMemcpyAsync(mesh_dir_out, S.mesh_dir, 12 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (cost_out) HIPCHK(hipMemcpyAsync(cost_out, S.cost, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (cmd_out) HIPCHK(hipMemcpyAsync(cmd_out, S.cmd, 16 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (how_out) HIPCHK(hipMemcpyAsync(how_out, S.how, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (n_gl) S.ms_kernels += ev_ms(G.ev[2], G.ev[3]);
  S.stayed = cnt[2]; S.neighbour = cnt[3]; S.global = cnt[4]; S.lost = cnt[6]; S.no_field = cnt[7];   // (cnt[5], reached: the rollout's)
  S.ms_total = (float)(1e-3 * (double)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count());
  return 0;
}

int mnav_follow_stats(const mnav_ctx* ctx, uint32_t* stayed, uint32_t* neighbour, uint32_t* global, uint32_t* lost, uint32_t* no_field,
                      uint32_t* built_index, float* ms_kernels, float* ms_total)
{
  if (!ctx) return -1;
  const mnav_fol::State& S = ctx->fol;
  if (stayed) *stayed = S.stayed;
  if (neighbour) *neighbour = S.neighbour;
  if (global) *global = S.global;
  if (lost) *lost = S.lost;
  if (no_field) *no_field = S.no_field;
  if (built_index) *built_index = S.built_index;
  if (ms_kernels) *ms_kernels = S.ms_kernels;
  if (ms_total) *ms_total = S.ms_total;
  return 0;
}
