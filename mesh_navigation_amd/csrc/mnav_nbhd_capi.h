// mnav_nbhd_capi.h -- the C ABI of the local-neighbourhood layers (include/mnav.h: mnav_layer_height_diff,
// mnav_layer_roughness, mnav_layer_ridge, mnav_neighbourhood_stats).  Included by mnav.hip inside its extern "C" block,
// after mnav_ctx and the host helpers.
#pragma once

extern "C++" {
template <int OP>
static int nbhd_launch(mnav_ctx* ctx, mnav_ctx::Layer& L, const mnav_nb::Mesh& M, uint32_t* n_spilled)
{
  using namespace mnav_nb;
  State& S = ctx->nbhd;
  const uint32_t V = ctx->V;
  if (!S.cnt)
    HIPCHK(alloc_group(S.cnt, sizeof(uint32_t) * (kCounters32 + 2), S.list[0], sizeof(uint32_t) * (V ? V : 1), S.list[1], sizeof(uint32_t) * (V ? V : 1)));
  // LDS passes: all centres with `cap` members per group, then (default only) the spill list with kWideLdsCap; an
  // explicit nbhd_lds_cap makes its pass the only LDS pass (tests reach the global spill path with it)
  const bool wide = !opt_set(ctx->opt.nbhd_lds_cap);
  uint32_t cap = opt_u32(ctx->opt.nbhd_lds_cap, kDefaultLdsCap);
  cap = cap < 2 * mnav_nb::kGroup ? 2 * mnav_nb::kGroup : (cap > kWideLdsCap ? kWideLdsCap : cap);   // >= 2 rounds of inserts: the hash
                                                                  // set stays at most 3/4 full; <= 512: 96 KiB of LDS per workgroup
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  HIPCHK(hipMemsetAsync(S.cnt, 0, sizeof(uint32_t) * (kCounters32 + 2), ctx->stream));
  uint32_t c[kCounters32];
  uint32_t n = V, in = 0;
  for (int pass = 0; pass < (wide ? 2 : 1) && n; ++pass) {
    const uint32_t pcap = pass ? kWideLdsCap : cap, ctr = pass ? kOverflow : kSpilled;
    uint32_t hsize = 1;
    while (hsize < 2 * pcap) hsize <<= 1;
    const size_t lds = sizeof(uint32_t) * (size_t)kCentresPerBlock * (hsize + pcap);
    if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_nbhd<OP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (pass) HIPCHK(hipMemsetAsync(S.cnt + kOverflow, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_nbhd<OP>, dim3((n + kCentresPerBlock - 1) / kCentresPerBlock), dim3(kNbBlock), lds, ctx->stream, M,
                       pass ? S.list[0] : nullptr, n, hsize - 1, pcap, L.cost, L.lethal, S.list[pass], S.cnt, ctr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c, S.cnt, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (!pass) *n_spilled = c[kSpilled];
    n = c[ctr];
    in = pass;
  }
  // spill passes: one wave per centre, state in global scratch; a centre that outgrows `scap` goes to the next pass with
  // 4x the capacity, and a capacity of at least V cannot overflow (a neighbourhood has at most V members)
  uint32_t scap = std::max<uint32_t>(8 * cap, 1024);
  while (n) {
    if (scap > V) scap = std::max<uint32_t>(V, 64);
    uint32_t sh = 1;
    while (sh < 2 * scap) sh <<= 1;
    const size_t per = (size_t)sh + scap;
    const size_t budget = (size_t)64 << 20;                        // words of scratch (256 MiB) shared by the pass's waves
    const uint32_t waves = (uint32_t)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(n, budget / per), 8192));
    if (S.scratch_words < per * waves) {
      S.scratch_words = 0;
      HIPCHK(S.scratch.alloc(sizeof(uint32_t) * per * waves));
      S.scratch_words = per * waves;
    }
    HIPCHK(hipMemsetAsync(S.cnt + kOverflow, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_nbhd_spill<OP>, dim3(waves), dim3(64), 0, ctx->stream, M, S.list[in], n, sh - 1, scap, S.scratch, L.cost, L.lethal,
                       S.list[in ^ 1], S.cnt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c, S.cnt, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (c[kOverflow] && scap >= V) { ctx->err = "neighbourhood visit: a centre overflowed a capacity of V"; return -1; }
    n = c[kOverflow];
    in ^= 1;
    scap = scap > V / 4 ? V : scap * 4;
  }
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  uint64_t visits = 0;
  HIPCHK(hipMemcpyAsync(&visits, S.cnt + kCounters32, sizeof(visits), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(c, S.cnt, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  S.visits = visits;
  S.max_size = c[kMaxSize];
  S.ms = ev_ms(ctx->ev[0], ctx->ev[1]);
  return 0;
}
}  // extern "C++"

// the three entry points share everything but the reduction and the normals they read
static int nbhd_layer(mnav_ctx* ctx, int op, uint32_t layer, double radius, double threshold)
{
  using namespace mnav_nb;
  if (!ctx) return -1;
  ctx->err.clear();
  if (!std::isfinite(radius) || radius < 0.0) { ctx->err = "radius must be finite and >= 0"; return -1; }
  if (!ctx->have_mesh) { ctx->err = "mnav_upload_mesh has not been called"; return -1; }
  if (layer >= 64) { ctx->err = "layer index out of range (64 layers)"; return -1; }
  if (op != kHeight && !ctx->have_normals) { ctx->err = "vertex normals are not resident (mnav_upload_mesh with vertex_normals)"; return -1; }
  // a ridge term is at most 2 * radius + 2 for unit normals: the int64 sum of 2^32-scaled terms must stay below 2^63
  if (op == kRidge && (double)ctx->V * (2.0 * radius + 2.0) >= 2147483648.0) { ctx->err = "ridge: V * (2 * radius + 2) must stay below 2^31"; return -1; }
  if (layer_slot(ctx, layer, false)) return -1;
  mnav_ctx::Layer& L = ctx->layers[layer];
  const Mesh M{ ctx->d_row_ptr, ctx->d_nbr_u, ctx->d_xyz, ctx->d_nrm, ctx->V, radius * radius, threshold };
  uint32_t spilled = 0;
  const int rc = op == kHeight ? nbhd_launch<kHeight>(ctx, L, M, &spilled)
               : op == kRough ? nbhd_launch<kRough>(ctx, L, M, &spilled) : nbhd_launch<kRidge>(ctx, L, M, &spilled);
  if (rc) return rc;
  layer_commit_plain(L);
  ctx->nbhd.centres = ctx->V;
  ctx->nbhd.spilled = spilled;
  return 0;
}

int mnav_layer_height_diff(mnav_ctx* ctx, uint32_t layer, double radius, double threshold)
{
  return nbhd_layer(ctx, mnav_nb::kHeight, layer, radius, threshold);
}

int mnav_layer_roughness(mnav_ctx* ctx, uint32_t layer, double radius, double threshold)
{
  return nbhd_layer(ctx, mnav_nb::kRough, layer, radius, threshold);
}

int mnav_layer_ridge(mnav_ctx* ctx, uint32_t layer, double radius, double threshold)
{
  return nbhd_layer(ctx, mnav_nb::kRidge, layer, radius, threshold);
}

int mnav_neighbourhood_stats(const mnav_ctx* ctx, uint32_t* centres, uint64_t* visits, uint32_t* max_size, uint32_t* spilled, float* ms)
{
  if (!ctx) return -1;
  const mnav_nb::State& S = ctx->nbhd;
  if (centres) *centres = S.centres;
  if (visits) *visits = S.visits;
  if (max_size) *max_size = S.max_size;
  if (spilled) *spilled = S.spilled;
  if (ms) *ms = S.ms;
  return 0;
}
