// mnav_obstacle_capi.h -- the C ABI of the obstacle layer (include/mnav.h: mnav_layer_obstacle, mnav_obstacle_stats) and
// the lazy BVH build behind it.  Included by mnav.hip inside its extern "C" block, after mnav_ctx and the host helpers.
#pragma once

// Karras 2012 LBVH over the resident faces: bounds -> Morton codes -> radix sort -> hierarchy -> leaves + refit.
static int obstacle_build_bvh(mnav_ctx* ctx)
{
  using namespace mnav_obs;
  Bvh& B = ctx->obs;
  const uint32_t F = ctx->F, V = ctx->V;
  HIPCHK(hipEventRecord(ctx->ev[4], ctx->stream));
  HIPCHK(B.fvtx.alloc(sizeof(uint32_t) * 3 * (size_t)(F ? F : 1)));
  if (F) HIPCHK(hipMemcpyAsync(B.fvtx, ctx->h_faces.data(), sizeof(uint32_t) * 3 * (size_t)F, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(B.tris.alloc(sizeof(float4) * 3 * (size_t)(F ? F : 1)));
  HIPCHK(B.nodes.alloc(sizeof(float4) * 4 * (size_t)(F > 1 ? F - 1 : 1)));
  if (F) {
    DevBuf<uint32_t> bnd, keys, keys2, ids, ids2, par_int, par_leaf, arrive;
    DevBuf<uint8_t> tmp;
    HIPCHK(bnd.alloc(6 * sizeof(uint32_t)));
    HIPCHK(keys.alloc(sizeof(uint32_t) * F)); HIPCHK(keys2.alloc(sizeof(uint32_t) * F));
    HIPCHK(ids.alloc(sizeof(uint32_t) * F)); HIPCHK(ids2.alloc(sizeof(uint32_t) * F));
    HIPCHK(par_int.alloc(sizeof(uint32_t) * F)); HIPCHK(par_leaf.alloc(sizeof(uint32_t) * F));
    HIPCHK(arrive.alloc(sizeof(uint32_t) * F));
    HIPCHK(hipMemsetAsync(bnd, 0xFF, 3 * sizeof(uint32_t), ctx->stream));
    HIPCHK(hipMemsetAsync((uint32_t*)bnd + 3, 0, 3 * sizeof(uint32_t), ctx->stream));
    HIPCHK(hipMemsetAsync(arrive, 0, sizeof(uint32_t) * F, ctx->stream));
    HIPCHK(hipMemsetAsync(par_int, 0xFF, sizeof(uint32_t) * F, ctx->stream));
    HIPCHK(hipMemsetAsync(par_leaf, 0xFF, sizeof(uint32_t) * F, ctx->stream));
    const uint32_t gv = (V + 255) / 256;
    hipLaunchKernelGGL(k_obs_bounds, dim3(gv < 1024 ? (gv ? gv : 1) : 1024), dim3(256), 0, ctx->stream, V, ctx->d_xyz, bnd);
    const uint32_t gf = (F + 255) / 256;
    hipLaunchKernelGGL(k_obs_morton, dim3(gf), dim3(256), 0, ctx->stream, F, B.fvtx, ctx->d_xyz, bnd, keys, ids);
    HIPCHK(hipGetLastError());
    size_t tmp_bytes = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, (uint32_t*)keys, (uint32_t*)keys2, (uint32_t*)ids, (uint32_t*)ids2, F, 0, 30, ctx->stream));
    HIPCHK(tmp.alloc(tmp_bytes ? tmp_bytes : 1));
    HIPCHK(rocprim::radix_sort_pairs((void*)tmp, tmp_bytes, (uint32_t*)keys, (uint32_t*)keys2, (uint32_t*)ids, (uint32_t*)ids2, F, 0, 30, ctx->stream));
    if (F > 1)
      hipLaunchKernelGGL(k_obs_hierarchy<uint32_t>, dim3((F - 1 + 255) / 256), dim3(256), 0, ctx->stream, F, keys2, B.nodes, par_int, par_leaf);
    hipLaunchKernelGGL(k_obs_leaves, dim3(gf), dim3(256), 0, ctx->stream, F, ids2, B.fvtx, ctx->d_xyz, B.tris, B.nodes, par_int, par_leaf, arrive);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev[5], ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));                   // the temporaries go out of scope
  } else {
    HIPCHK(hipEventRecord(ctx->ev[5], ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  B.F = F;
  B.root = F > 1 ? 0u : (F == 1 ? kLeaf : kNone);
  B.ms_build = ev_ms(ctx->ev[4], ctx->ev[5]);
  B.valid = true;
  return 0;
}

// the argument errors of mnav_layer_obstacle (and mnav_map_obstacle): refused before anything is touched
static int obstacle_check_args(mnav_ctx* ctx, uint32_t n_points, const void* points, uint32_t point_step, const float* down_axis)
{
  if (point_step < 12) { ctx->err = "point_step must be at least 12 bytes (x, y, z floats at offsets 0, 4, 8)"; return -1; }
  if (n_points && !points) { ctx->err = "null point buffer with n_points > 0"; return -1; }
  if (!down_axis) { ctx->err = "null down_axis"; return -1; }
  if (!std::isfinite(down_axis[0]) || !std::isfinite(down_axis[1]) || !std::isfinite(down_axis[2]) ||
      (down_axis[0] == 0.f && down_axis[1] == 0.f && down_axis[2] == 0.f)) { ctx->err = "down_axis must be finite and non-zero"; return -1; }
  return 0;
}

int mnav_layer_obstacle(mnav_ctx* ctx, uint32_t layer, uint32_t n_points, const void* points, uint32_t point_step,
                        const float* sensor_to_map, const float* down_axis, double robot_height, double max_obstacle_dist,
                        uint32_t* changed_out, uint32_t* n_changed, uint32_t* n_lethal)
{
  using namespace mnav_obs;
  using namespace mnav_chg;
  if (!ctx) return -1;
  ctx->err.clear();
  if (obstacle_check_args(ctx, n_points, points, point_step, down_axis)) return -1;
  if (layer_slot(ctx, layer, false)) return -1;
  mnav_ctx::Layer& L = ctx->layers[layer];
  Bvh& B = ctx->obs;
  const uint32_t V = ctx->V;
  if (!B.valid && obstacle_build_bvh(ctx)) { B = Bvh{}; return -1; }
  if (!B.flags) HIPCHK(B.flags.alloc(V ? V : 1));
  if (change_scratch(ctx)) return -1;
  uint32_t* const cnt = ctx->chg.cnt;
  const size_t bytes = (size_t)n_points * point_step;
  if (bytes > B.pts_cap) {
    B.pts_cap = 0;
    HIPCHK(B.pts.alloc(bytes));
    B.pts_cap = bytes;
  }
  CastArgs A{};
  A.n = n_points; A.step = point_step; A.F = B.F; A.root = B.root;
  static const float kIdentity[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
  std::memcpy(A.m, sensor_to_map ? sensor_to_map : kIdentity, sizeof(A.m));
  A.rs = ray_setup(down_axis[0], down_axis[1], down_axis[2]);
  for (int a = 0; a < 3; ++a) A.inv[a] = ray_slab_inverse(down_axis[a]);
  A.max_dist = max_obstacle_dist; A.robot_height = robot_height;
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  if (!L.ready) HIPCHK(hipMemsetAsync(L.lethal, 0, V ? V : 1, ctx->stream));   // a fresh slot: the old set is empty
  HIPCHK(hipMemsetAsync(B.flags, 0, V ? V : 1, ctx->stream));
  HIPCHK(hipMemsetAsync(cnt, 0, sizeof(uint32_t) * kCounters, ctx->stream));
  if (bytes) HIPCHK(hipMemcpyAsync(B.pts, points, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  if (n_points) hipLaunchKernelGGL(k_obs_cast, dim3((n_points + kCastBlock - 1) / kCastBlock), dim3(kCastBlock), 0, ctx->stream, A, B.pts,
                                   B.nodes, B.tris, B.fvtx, B.flags, cnt);
  HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
  uint32_t c[kCounters];
  if (layer_change_list(ctx, L, FlagRule{ B.flags }, ctx->ev[3], c, changed_out, n_changed, n_lethal)) return -1;
  B.kept = c[kKept]; B.hits = c[kHits]; B.lethal_rays = c[kLethalRays];
  B.ms_cast = ev_ms(ctx->ev[1], ctx->ev[2]);
  B.ms_total = ev_ms(ctx->ev[0], ctx->ev[3]);
  if (c[kOverflow]) { ctx->err = "obstacle ray cast: BVH traversal stack overflow"; return -1; }
  return 0;
}

int mnav_obstacle_stats(const mnav_ctx* ctx, uint32_t* rays_kept, uint32_t* hits, uint32_t* lethal_rays, float* ms_bvh_build,
                        float* ms_cast, float* ms_total)
{
  if (!ctx) return -1;
  const mnav_obs::Bvh& B = ctx->obs;
  if (rays_kept) *rays_kept = B.kept;
  if (hits) *hits = B.hits;
  if (lethal_rays) *lethal_rays = B.lethal_rays;
  if (ms_bvh_build) *ms_bvh_build = B.ms_build;
  if (ms_cast) *ms_cast = B.ms_cast;
  if (ms_total) *ms_total = B.ms_total;
  return 0;
}
