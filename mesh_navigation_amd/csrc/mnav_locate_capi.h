// mnav_locate_capi.h -- the C ABI of the pose lookup (include/mnav.h: mnav_locate, mnav_locate_stats and the two plan
// entry points that start from positions) and the lazy index build behind it.  Included by mnav.hip inside its
// extern "C" block, after mnav_ctx and the host helpers.
#pragma once

// bounds -> keys -> radix sort -> points + leaf keys -> Karras hierarchy over the leaves -> boxes bottom-up
static int locate_build(mnav_ctx* ctx)
{
  using namespace mnav_loc;
  State& S = ctx->loc;
  const uint32_t V = ctx->V;
  if (upload_walk_mesh(ctx)) return -1;
  HIPCHK(hipEventRecord(ctx->ev[4], ctx->stream));
  uint32_t n_pts = 0;
  DevBuf<uint64_t> keys, keys2, leaf_keys;
  DevBuf<uint32_t> ids, ids2, par_int, par_leaf, arrive, cnt, bnd;
  DevBuf<uint8_t> tmp;
  if (V) {
    HIPCHK(keys.alloc(sizeof(uint64_t) * V)); HIPCHK(keys2.alloc(sizeof(uint64_t) * V));
    HIPCHK(ids.alloc(sizeof(uint32_t) * V)); HIPCHK(ids2.alloc(sizeof(uint32_t) * V));
    HIPCHK(cnt.alloc(sizeof(uint32_t))); HIPCHK(bnd.alloc(6 * sizeof(uint32_t)));
    HIPCHK(hipMemsetAsync(cnt, 0, sizeof(uint32_t), ctx->stream));
    HIPCHK(hipMemsetAsync(bnd, 0xFF, 3 * sizeof(uint32_t), ctx->stream));
    HIPCHK(hipMemsetAsync((uint32_t*)bnd + 3, 0, 3 * sizeof(uint32_t), ctx->stream));
    const uint32_t gv = (V + 255) / 256;
    hipLaunchKernelGGL(k_loc_bounds, dim3(gv < 1024 ? gv : 1024), dim3(256), 0, ctx->stream, V, ctx->d_xyz, bnd);
    hipLaunchKernelGGL(k_loc_keys, dim3(gv), dim3(256), 0, ctx->stream, V, ctx->d_xyz, bnd, keys, ids, cnt);
    HIPCHK(hipGetLastError());
    size_t tmp_bytes = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, (uint64_t*)keys, (uint64_t*)keys2, (uint32_t*)ids, (uint32_t*)ids2, V, 0, 64, ctx->stream));
    HIPCHK(tmp.alloc(tmp_bytes ? tmp_bytes : 1));
    HIPCHK(rocprim::radix_sort_pairs((void*)tmp, tmp_bytes, (uint64_t*)keys, (uint64_t*)keys2, (uint32_t*)ids, (uint32_t*)ids2, V, 0, 64, ctx->stream));
    HIPCHK(hipMemcpyAsync(&n_pts, cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (n_pts > V) { ctx->err = "locate index: vertex count out of range"; return -1; }
  }
  const uint32_t n_leaves = (n_pts + kRun - 1) / kRun;
  HIPCHK(S.pts.alloc(sizeof(F4) * kRun * (size_t)(n_leaves ? n_leaves : 1)));
  HIPCHK(S.nodes.alloc(sizeof(F4) * 4 * (size_t)(n_leaves > 1 ? n_leaves - 1 : 1)));
  if (n_pts) {
    HIPCHK(leaf_keys.alloc(sizeof(uint64_t) * n_leaves));
    HIPCHK(par_int.alloc(sizeof(uint32_t) * n_leaves)); HIPCHK(par_leaf.alloc(sizeof(uint32_t) * n_leaves));
    HIPCHK(arrive.alloc(sizeof(uint32_t) * n_leaves));
    HIPCHK(hipMemsetAsync(arrive, 0, sizeof(uint32_t) * n_leaves, ctx->stream));
    HIPCHK(hipMemsetAsync(par_int, 0xFF, sizeof(uint32_t) * n_leaves, ctx->stream));
    HIPCHK(hipMemsetAsync(par_leaf, 0xFF, sizeof(uint32_t) * n_leaves, ctx->stream));
    hipLaunchKernelGGL(k_loc_points, dim3((n_leaves * kRun + 255) / 256), dim3(256), 0, ctx->stream, n_pts, n_leaves, ids2, keys2, ctx->d_xyz, S.pts, leaf_keys);
    if (n_leaves > 1) {
      hipLaunchKernelGGL(mnav_obs::k_obs_hierarchy<uint64_t>, dim3((n_leaves - 1 + 255) / 256), dim3(256), 0, ctx->stream, n_leaves, leaf_keys,
                         (float4*)S.nodes.get(), par_int, par_leaf);
      hipLaunchKernelGGL(k_loc_refit, dim3((n_leaves + 255) / 256), dim3(256), 0, ctx->stream, n_pts, n_leaves, S.pts, S.nodes, par_int, par_leaf, arrive);
    }
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(ctx->ev[5], ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));                     // the temporaries go out of scope
  S.n_pts = n_pts; S.n_leaves = n_leaves;
  S.ms_build = ev_ms(ctx->ev[4], ctx->ev[5]);
  S.valid = true;
  return 0;
}

// The index for a call that needs one: built if the context has none (nothing is kept of a build that failed) and then
// reported by mnav_locate_stats as the lookup's own; *built = 1 when this call built it.
static int locate_ensure(mnav_ctx* ctx, uint32_t* built)
{
  mnav_loc::State& S = ctx->loc;
  if (S.valid) return 0;
  if (locate_build(ctx)) { S.nodes.reset(); S.pts.reset(); S.valid = false; return -1; }
  S.built = 1; *built = 1;
  return 0;
}

// n_a + n_b queries (two host arrays, either may be empty) through the index; the results stay in S.vtx / face / bary / dist
static int locate_run(mnav_ctx* ctx, uint32_t n_a, const float* pos_a, uint32_t n_b, const float* pos_b)
{
  using namespace mnav_loc;
  State& S = ctx->loc;
  S.built = 0; S.ms_query = 0.f; S.candidates = 0;
  if (!ctx->have_mesh) { ctx->err = "mnav_upload_mesh has not been called"; return -1; }
  if ((n_a && !pos_a) || (n_b && !pos_b)) { ctx->err = "null position array"; return -1; }
  const size_t n = (size_t)n_a + n_b;
  if (n > 0x7FFFFFFFu) { ctx->err = "too many positions in one call"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  if (locate_ensure(ctx, &S.built)) return -1;
  if (!n) return 0;
  if (n > S.cap) {
    S.cap = 0;
    if (alloc_group(S.q, 12 * n, S.bary, 12 * n, S.dist, 4 * n, S.vtx, 4 * n, S.face, 4 * n) != hipSuccess) { ctx->err = "locate: out of device memory"; return -1; }
    S.cap = n;
  }
  if (!S.cnt) HIPCHK(S.cnt.alloc(sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(S.cnt, 0, sizeof(unsigned long long), ctx->stream));
  if (n_a) HIPCHK(hipMemcpyAsync(S.q, pos_a, 12 * (size_t)n_a, hipMemcpyHostToDevice, ctx->stream));
  if (n_b) HIPCHK(hipMemcpyAsync(S.q + 3 * (size_t)n_a, pos_b, 12 * (size_t)n_b, hipMemcpyHostToDevice, ctx->stream));
  const Index I{ S.nodes, S.pts, S.n_pts, S.n_leaves, loc_root(S.n_leaves) };
  const WalkMesh M{ ctx->d_xyz, ctx->d_faces, ctx->d_vf_ptr, ctx->d_vf, ctx->V, ctx->F };
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  hipLaunchKernelGGL(k_loc_query, dim3((uint32_t)((n + kLocBlock - 1) / kLocBlock)), dim3(kLocBlock), 0, ctx->stream, (uint32_t)n, S.q, I, M, S.vtx, S.face,
                     S.bary, S.dist, S.cnt);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  unsigned long long cand = 0;
  HIPCHK(hipMemcpyAsync(&cand, S.cnt, sizeof(cand), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  S.candidates = cand;
  S.ms_query = ev_ms(ctx->ev[0], ctx->ev[1]);
  return 0;
}

int mnav_locate(mnav_ctx* ctx, uint32_t n, const float* pos, uint32_t* vertex_out, uint32_t* face_out, float* bary_out, float* dist_out)
{
  if (!ctx) return -1;
  ctx->err.clear();
  if (!n) return 0;
  if (locate_run(ctx, n, pos, 0, nullptr)) return -1;
  const mnav_loc::State& S = ctx->loc;
  if (vertex_out) HIPCHK(hipMemcpyAsync(vertex_out, S.vtx, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (face_out) HIPCHK(hipMemcpyAsync(face_out, S.face, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (bary_out) HIPCHK(hipMemcpyAsync(bary_out, S.bary, 12 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (dist_out) HIPCHK(hipMemcpyAsync(dist_out, S.dist, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mnav_locate_stats(const mnav_ctx* ctx, uint32_t* built, float* ms_build, float* ms_query, uint64_t* candidates)
{
  if (!ctx) return -1;
  const mnav_loc::State& S = ctx->loc;
  if (built) *built = S.built;
  if (ms_build) *ms_build = S.ms_build;
  if (ms_query) *ms_query = S.ms_query;
  if (candidates) *candidates = S.candidates;
  return 0;
}

// goal and start positions -> ids (`faces`: the containing faces, else the nearest vertices); only the 2n ids come down
static int locate_ends(mnav_ctx* ctx, uint32_t n, const float* goal_pos, const float* start_pos, bool faces, std::vector<uint32_t>& goal_ids,
                       std::vector<uint32_t>& start_ids)
{
  if (locate_run(ctx, n, goal_pos, n, start_pos)) return -1;
  goal_ids.resize(n); start_ids.resize(n);
  const uint32_t* src = faces ? ctx->loc.face : ctx->loc.vtx;
  HIPCHK(hipMemcpyAsync(goal_ids.data(), src, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(start_ids.data(), src + n, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

uint32_t mnav_plan_dijkstra_batch_at(mnav_ctx* ctx, uint32_t n, const float* goal_pos, const float* start_pos, double goal_dist_offset,
                                     double cost_limit, uint32_t* codes_out, uint32_t* seeds_out, uint32_t* targets_out, float* dist_out,
                                     uint32_t* pred_out, uint32_t* path_out, uint32_t path_cap, uint32_t* path_len)
{
  if (!ctx) return MNAV_INTERNAL_ERROR;
  if (n == 0) return MNAV_SUCCESS;
  ctx->err.clear();
  if (!goal_pos || !start_pos) { ctx->err = "null goal/start positions"; return MNAV_INTERNAL_ERROR; }
  if (check_ready(ctx)) return MNAV_INTERNAL_ERROR;                   // before the lookup: a call that cannot plan changes nothing
  std::vector<uint32_t> seeds, targets;
  if (locate_ends(ctx, n, goal_pos, start_pos, false, seeds, targets)) return MNAV_INTERNAL_ERROR;
  if (seeds_out) std::memcpy(seeds_out, seeds.data(), 4 * (size_t)n);
  if (targets_out) std::memcpy(targets_out, targets.data(), 4 * (size_t)n);
  return mnav_plan_dijkstra_batch(ctx, n, seeds.data(), targets.data(), goal_dist_offset, cost_limit, codes_out, dist_out, pred_out, path_out,
                                  path_cap, path_len);
}

uint32_t mnav_plan_cvp_batch_at(mnav_ctx* ctx, uint32_t n, const float* goal_pos, const float* start_pos, double goal_dist_offset,
                                double cost_limit, uint32_t* codes_out, uint32_t* seed_faces_out, uint32_t* target_faces_out, float* dist_out,
                                uint32_t* pred_out, float* vecmap_out)
{
  if (!ctx) return MNAV_INTERNAL_ERROR;
  if (n == 0) return MNAV_SUCCESS;
  ctx->err.clear();
  if (!goal_pos || !start_pos) { ctx->err = "null goal/start positions"; return MNAV_INTERNAL_ERROR; }
  if (check_ready(ctx)) return MNAV_INTERNAL_ERROR;
  std::vector<uint32_t> seed_faces, target_faces;
  if (locate_ends(ctx, n, goal_pos, start_pos, true, seed_faces, target_faces)) return MNAV_INTERNAL_ERROR;
  if (seed_faces_out) std::memcpy(seed_faces_out, seed_faces.data(), 4 * (size_t)n);
  if (target_faces_out) std::memcpy(target_faces_out, target_faces.data(), 4 * (size_t)n);
  return mnav_plan_cvp_batch(ctx, n, goal_pos, seed_faces.data(), target_faces.data(), goal_dist_offset, cost_limit, codes_out, dist_out, pred_out,
                             vecmap_out);
}
