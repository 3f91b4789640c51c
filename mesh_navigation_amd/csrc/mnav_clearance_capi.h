// mnav_clearance_capi.h -- the C ABI of the clearance and border layers (include/mnav.h: mnav_layer_clearance,
// mnav_layer_border, mnav_clearance_download, mnav_clearance_stats).  Included by mnav.hip inside its extern "C" block,
// after mnav_ctx, the host helpers and mnav_obstacle_capi.h (obstacle_build_bvh).
#pragma once

// the clearance of every vertex into the cache: the BVH (unless an obstacle call built it), then one ray per vertex.  On
// any failure the cache stays invalid.
static int clr_cast(mnav_ctx* ctx)
{
  using namespace mnav_clr;
  using namespace mnav_chg;
  State& S = ctx->clr;
  mnav_obs::Bvh& B = ctx->obs;
  const uint32_t V = ctx->V;
  S.valid = false;
  S.ms_build = 0.f;
  if (!B.valid) {
    if (obstacle_build_bvh(ctx)) { B = mnav_obs::Bvh{}; return -1; }
    S.ms_build = B.ms_build;
  }
  if (!S.clr) HIPCHK(S.clr.alloc(sizeof(float) * (V ? V : 1)));
  if (change_scratch(ctx)) return -1;
  uint32_t* const cnt = ctx->chg.cnt;
  const CastArgs A{ V, B.F, B.root, ctx->d_xyz, ctx->d_nrm };
  HIPCHK(hipMemsetAsync(cnt, 0, sizeof(uint32_t) * kCounters, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  const uint32_t wave = mnav_obs::kCastBlock;
  if (V) hipLaunchKernelGGL(k_clr_cast, dim3((V + wave - 1) / wave), dim3(wave), 0, ctx->stream, A, B.nodes, B.tris, B.fvtx, S.clr, cnt);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  uint32_t c[kCounters];
  HIPCHK(hipMemcpyAsync(c, cnt, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  S.rays = c[kKept]; S.hits = c[kHits];
  S.ms_cast = ev_ms(ctx->ev[0], ctx->ev[1]);
  if (c[kOverflow]) { ctx->err = "clearance ray cast: BVH traversal stack overflow"; return -1; }
  S.valid = true;
  return 0;
}

int mnav_layer_clearance(mnav_ctx* ctx, uint32_t layer, double robot_height, double height_inflation, uint32_t* changed_out,
                         uint32_t* n_changed, uint32_t* n_lethal)
{
  using namespace mnav_clr;
  if (!ctx) return -1;
  ctx->err.clear();
  if (!ctx->have_mesh) { ctx->err = "mnav_upload_mesh has not been called"; return -1; }
  if (!std::isfinite(robot_height) || !std::isfinite(height_inflation) || robot_height < 0.0 || height_inflation < 0.0) {
    ctx->err = "robot_height and height_inflation must be finite and >= 0";
    return -1;
  }
  if (layer >= 64) { ctx->err = "layer index out of range (64 layers)"; return -1; }
  if (!ctx->have_normals) { ctx->err = "vertex normals are not resident (mnav_upload_mesh with vertex_normals)"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  State& S = ctx->clr;
  HIPCHK(hipEventRecord(ctx->ev[6], ctx->stream));
  S.cast = S.valid ? 0u : 1u;
  if (!S.valid) {
    if (clr_cast(ctx)) return -1;                                  // the slot is not touched before the cast succeeded
  } else {
    S.rays = S.hits = 0;
    S.ms_build = S.ms_cast = 0.f;
  }
  if (layer_slot(ctx, layer, false)) return -1;
  uint32_t c[mnav_chg::kCounters];
  const ClearanceRule rule{ S.clr, robot_height, height_inflation };
  if (layer_change_list(ctx, ctx->layers[layer], rule, ctx->ev[7], c, changed_out, n_changed, n_lethal)) return -1;
  S.ms_total = ev_ms(ctx->ev[6], ctx->ev[7]);
  return 0;
}

int mnav_layer_border(mnav_ctx* ctx, uint32_t layer, double border_cost, double threshold, uint32_t* changed_out, uint32_t* n_changed,
                      uint32_t* n_lethal)
{
  using namespace mnav_clr;
  if (!ctx) return -1;
  ctx->err.clear();
  if (!ctx->have_mesh) { ctx->err = "mnav_upload_mesh has not been called"; return -1; }
  if (!std::isfinite(border_cost)) { ctx->err = "border_cost must be finite"; return -1; }
  if (std::isnan(threshold)) { ctx->err = "threshold must not be NaN"; return -1; }
  if (layer_slot(ctx, layer, false)) return -1;
  State& S = ctx->clr;
  const uint32_t V = ctx->V;
  if (!S.border) HIPCHK(S.border.alloc(V ? V : 1));
  if (V) hipLaunchKernelGGL(k_border, dim3((V + 255) / 256), dim3(256), 0, ctx->stream, V, ctx->d_row_ptr, ctx->d_nbr_e, ctx->d_crn_ptr,
                            ctx->d_crn_idx, S.border);
  HIPCHK(hipGetLastError());
  uint32_t c[mnav_chg::kCounters];
  return layer_change_list(ctx, ctx->layers[layer], BorderRule{ S.border, border_cost, threshold }, ctx->ev[7], c, changed_out, n_changed, n_lethal);
}

int mnav_clearance_download(const mnav_ctx* cctx, float* clearance_out)
{
  if (!cctx) return -1;
  mnav_ctx* ctx = const_cast<mnav_ctx*>(cctx);                      // the error string and the stream are the context's
  ctx->err.clear();
  if (!ctx->clr.valid) { ctx->err = "no clearance is cached (mnav_layer_clearance after mnav_upload_mesh)"; return -1; }
  if (!clearance_out) { ctx->err = "null clearance array"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  if (ctx->V) HIPCHK(hipMemcpyAsync(clearance_out, ctx->clr.clr, sizeof(float) * ctx->V, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mnav_clearance_stats(const mnav_ctx* ctx, uint32_t* cast, uint32_t* rays, uint32_t* hits, float* ms_bvh_build, float* ms_cast,
                         float* ms_total)
{
  if (!ctx) return -1;
  const mnav_clr::State& S = ctx->clr;
  if (cast) *cast = S.cast;
  if (rays) *rays = S.rays;
  if (hits) *hits = S.hits;
  if (ms_bvh_build) *ms_bvh_build = S.ms_build;
  if (ms_cast) *ms_cast = S.ms_cast;
  if (ms_total) *ms_total = S.ms_total;
  return 0;
}
