// mnav_tb_host.h -- host driver of the tile-batch SSSP engine (mnav_tb.h).  Included by mnav.hip inside its anonymous
// namespace, after mnav_ctx and the helpers (HIPCHK, ev_ms, PlanIn) are defined.
#pragma once

void tb_free_batch(mnav_ctx* ctx)
{
  TbState& S = ctx->tb;
  if (S.fill_stream) (void)hipStreamSynchronize(S.fill_stream);      // (its fill may still be writing D2)
  static_cast<TbBatch&>(S) = TbBatch{};
  S.count_pending = false; ctx->tb_args_valid = false;               // the last batch's arguments point into freed memory now
  ctx->res.batch_state_freed();                                       // (the map of unreached pairs went with it)
}

void tb_free(mnav_ctx* ctx)
{
  tb_free_batch(ctx);
  static_cast<TbTables&>(ctx->tb) = TbTables{};
}

// mesh-dependent streams: built on the first batch that takes this engine (a few seconds of host work at 1M vertices)
int tb_build(mnav_ctx* ctx)
{
  TbState& S = ctx->tb;
  if (S.built) return 0;
  if (opt_set(ctx->opt.tb_tile)) S.T = opt_u32(ctx->opt.tb_tile, S.T);
  if (S.T != 64 && S.T != 96 && S.T != 120 && S.T != 128) S.T = 120;
  HostTopology t;
  t.V = ctx->V; t.E = ctx->E; t.F = ctx->F;
  t.row_ptr = ctx->h_row_ptr; t.nbr_u = ctx->h_nbr_u;
  HostTb H;
  try { H = build_tb(t, ctx->h_xyz.data(), S.T); }
  catch (const std::exception& ex) { ctx->err = ex.what(); return -1; }
  std::vector<uint2> vaddr(ctx->V);
  for (uint32_t v = 0; v < ctx->V; ++v) {
    const TbTile& W = H.tiles[H.vert_tile[v]];
    if (W.sl >= (1u << 24)) { ctx->err = "tile-batch engine: a tile has too many ghosts"; return -1; }
    vaddr[v] = make_uint2(W.soff, (W.sl << 8) | H.vert_local[v]);
  }
  HIPCHK(S.d_tiles.upload(ctx->stream, H.tiles.data(), H.tiles.size()));
  HIPCHK(S.d_stream.upload(ctx->stream, H.stream.data(), H.stream.size()));
  HIPCHK(S.d_wsrc.upload(ctx->stream, H.wsrc.data(), H.wsrc.size()));
  HIPCHK(S.d_exps.upload(ctx->stream, H.exps.data(), H.exps.size()));
  HIPCHK(S.d_vstream.upload(ctx->stream, H.vstream.data(), H.vstream.size()));
  HIPCHK(S.d_vwsrc.upload(ctx->stream, H.vwsrc.data(), H.vwsrc.size()));
  HIPCHK(S.d_vtile.upload(ctx->stream, H.vtile.data(), H.vtile.size()));
  if (H.vgroups.empty()) H.vgroups.push_back(0u);
  HIPCHK(S.d_vgroups.upload(ctx->stream, H.vgroups.data(), H.vgroups.size()));
  HIPCHK(S.d_vexps.upload(ctx->stream, H.vexps.data(), H.vexps.size()));
  HIPCHK(S.d_vaddr.upload(ctx->stream, vaddr.data(), vaddr.size()));
  HIPCHK(S.d_vert_tile.upload(ctx->stream, H.vert_tile.data(), H.vert_tile.size()));
  HIPCHK(S.d_verts.upload(ctx->stream, H.verts.data(), H.verts.size()));
  // finalize tables (mnav_tb_finalize.h)
  HIPCHK(S.d_fin_src.upload(ctx->stream, H.fin_src.data(), H.fin_src.size()));
  HIPCHK(S.d_fin_wsrc.upload(ctx->stream, H.fin_wsrc.data(), H.fin_wsrc.size()));
  HIPCHK(S.d_fin_ovf.upload(ctx->stream, H.fin_ovf.data(), H.fin_ovf.size()));
  {
    std::vector<uint32_t> ow(H.fin_ovf.size());
    for (size_t i = 0; i < ow.size(); ++i) ow[i] = H.fin_ovf[i].wsrc;
    HIPCHK(S.d_fin_ovf_wsrc.upload(ctx->stream, ow.data(), ow.size()));
  }
  HIPCHK(S.d_ghost_gid.upload(ctx->stream, H.ghost_gid.data(), H.ghost_gid.size()));
  {
    // k_tb_finalize's workgroups take the tiles in the order of their smallest vertex id: the tiles of a workgroup -- and of the
    // workgroups running next to it -- then write neighbouring pieces of the vertex-order output arrays (on a row-major grid: a
    // strip of tiles side by side, whose 11-vertex runs join to whole cache lines in the L2)
    std::vector<uint32_t> order(H.tiles.size()), key(H.tiles.size(), 0xFFFFFFFFu);
    for (size_t t = 0; t < H.tiles.size(); ++t) {
      order[t] = (uint32_t)t;
      for (uint32_t i = 0; i < H.tiles[t].nv; ++i) key[t] = std::min(key[t], H.verts[H.tiles[t].v0 + i]);
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    if (order.empty()) order.push_back(0u);
    HIPCHK(S.d_fin_order.upload(ctx->stream, order.data(), order.size()));
  }
  S.d_fin_w.reset(); S.d_fin_ovf_w.reset();
  S.fin_n = H.fin_src.size(); S.fin_novf = H.fin_ovf.size(); S.fin_w_valid = false; S.max_sl = H.max_sl;
  HIPCHK(S.d_fin_w.alloc(4 * std::max<size_t>(S.fin_n, 1)));
  HIPCHK(S.d_fin_ovf_w.alloc(4 * std::max<size_t>(S.fin_novf, 1)));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  S.nvrec = H.vstream.size();
  S.ntiles = H.ntiles; S.S = H.S; S.nrec = H.stream.size(); S.nexp = H.exps.size(); S.max_nh = H.max_nh;
  S.vert_tile = std::move(H.vert_tile);
  S.built = true; S.w_valid = false;
  if (opt_on(ctx->opt.verbose))
    fprintf(stderr, "[mnav] tile-batch engine: T %u, %u tiles, %.2f slots per vertex, max ghosts %u, %.1f MB of streams + %.1f MB of sweep streams in the V layout\n", S.T, S.ntiles,
            ctx->V ? (double)S.S / ctx->V : 0.0, S.max_nh, (4.0 * S.nrec + 16.0 * S.nexp) / 1e6, 4.0 * S.nvrec / 1e6);
  return 0;
}

int tb_weights(mnav_ctx* ctx)
{
  TbState& S = ctx->tb;
  if (S.w_valid) return 0;
  hipLaunchKernelGGL(k_tb_weights, dim3(4096), dim3(kBlock), 0, ctx->stream, S.nrec, S.d_wsrc, ctx->d_nbr, S.d_stream);
  hipLaunchKernelGGL(k_tb_weights, dim3(4096), dim3(kBlock), 0, ctx->stream, S.nvrec, S.d_vwsrc, ctx->d_nbr, S.d_vstream);
  HIPCHK(hipGetLastError());
  S.w_valid = true; S.fin_w_valid = false;
  return 0;
}

// weights of the finalize tables: like the streams' they follow the cost-limit folded gather CSR (w_valid is reset with it)
int tb_fin_weights(mnav_ctx* ctx)
{
  TbState& S = ctx->tb;
  if (S.fin_w_valid) return 0;
  hipLaunchKernelGGL(k_tb_fin_weights, dim3(4096), dim3(kBlock), 0, ctx->stream, S.fin_n, S.d_fin_wsrc, ctx->d_nbr, S.d_fin_w);
  if (S.fin_novf) hipLaunchKernelGGL(k_tb_fin_weights, dim3(64), dim3(kBlock), 0, ctx->stream, S.fin_novf, S.d_fin_ovf_wsrc, ctx->d_nbr, S.d_fin_ovf_w);
  HIPCHK(hipGetLastError());
  S.fin_w_valid = true;
  return 0;
}

int tb_ensure_batch(mnav_ctx* ctx, uint32_t np)
{
  TbState& S = ctx->tb;
  if (np <= S.cap_np) return 0;
  tb_free_batch(ctx);
  const size_t nt = S.ntiles ? S.ntiles : 1, pairs = nt * (size_t)np;
  HIPCHK(S.D.alloc(4 * (size_t)S.S * np + 64));
  S.umap_stride = (np + 63u) / 64u;                                   // (fixed by the capacity: a slot's bit stays where it is when the batch size changes)
  HIPCHK(S.umap.alloc(8 * nt * S.umap_stride)); HIPCHK(S.uskip.alloc(8 * nt * S.umap_stride)); HIPCHK(S.fin_cnt.alloc(16));
  HIPCHK(S.pend.alloc(4 * pairs + 64));
  HIPCHK(S.pflag.alloc(nt * (((size_t)np + 63) / 64) + 64));
  HIPCHK(S.bucket.alloc(2 * pairs + 64));
  HIPCHK(S.bcnt.alloc(4 * nt));
  HIPCHK(S.items.alloc(8 * (nt + pairs / kTbItemPlans + 64)));
  HIPCHK(S.ctl.alloc(sizeof(tb::Ctl)));
  HIPCHK(S.wstat.alloc(32 * (size_t)kTbStatSlots));
  HIPCHK(S.h_ctl.alloc(sizeof(tb::Ctl)));
  for (int k = 0; k < 2; ++k) HIPCHK(S.marr[k].alloc(4 * (size_t)np));
  HIPCHK(S.mcarry.alloc(4 * (size_t)kTbMinCopies * np + 64));
  HIPCHK(S.thr.alloc(4 * (size_t)np)); HIPCHK(S.bnd.alloc(4 * (size_t)np));
  HIPCHK(S.seed.alloc(4 * (size_t)np)); HIPCHK(S.target.alloc(4 * (size_t)np));
  HIPCHK(S.d_recs.alloc(sizeof(FinRec) * (size_t)np));
  HIPCHK(S.h_plans.alloc(sizeof(Plan) * (size_t)np)); HIPCHK(S.h_vecs.alloc(sizeof(float*) * (size_t)np));
  S.cap_np = np;
  return 0;
}

// The second distance buffer, its stream and its events: wanted by the calls that end without a finalize pass that resets D
// (tb_clean_other).  Optional: without it such a batch fills D at its start.
int tb_ensure_other(mnav_ctx* ctx)
{
  TbState& S = ctx->tb;
  if (S.D2 || 8 * (size_t)S.S * S.cap_np > ((size_t)96 << 30) || opt_on(ctx->opt.tb_no_prefill)) return 0;
  if (S.D2.alloc(4 * (size_t)S.S * S.cap_np + 64) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (!S.fill_stream) { HIPCHK(hipStreamCreateWithFlags(S.fill_stream.out(), hipStreamNonBlocking)); HIPCHK(hipEventCreateWithFlags(S.fill_done.out(), hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(S.call_done.out(), hipEventDisableTiming)); }
  S.d2_clean = false;
  return 0;
}

int tb_fill(mnav_ctx* ctx, void* p, size_t bytes, uint32_t v)
{
  const size_t n16 = (bytes + 15) / 16;                               // the buffers carry 64 bytes of slack
  uint32_t g = (uint32_t)std::min<size_t>((n16 + kBlock - 1) / kBlock, 256 * 32);
  if (g < 1) g = 1;
  hipLaunchKernelGGL(k_tb_fill, dim3(g), dim3(kBlock), 0, ctx->stream, (u32x4*)p, n16, v);
  HIPCHK(hipGetLastError());
  return 0;
}

int tb_launch_iterations(mnav_ctx* ctx, const tb::Args& A, int count, uint32_t waves)
{
  const uint32_t gp = (A.NP + kBlock - 1) / kBlock;
  const dim3 gs(std::max((A.ntiles + kTbSchedTiles - 1) / kTbSchedTiles, 1u)), bs(kTbSchedTiles * 64u);
  const size_t lds_s = A.sched_lds ? 4 * ((size_t)A.NP + 1u) : 0;   // (k_tb_sched: <= kTbSchedLdsMax, tb_sched_lds_fits)
  for (int j = 0; j < count; ++j) {
    const int par = j & 1;
    if (A.sched_lds) {
      hipLaunchKernelGGL((k_tb_plan<kTbMinCopiesLds>), dim3(gp), dim3(kBlock), 0, ctx->stream, A, par);
      hipLaunchKernelGGL((k_tb_sched<true>), gs, bs, lds_s, ctx->stream, A, par);
    } else {
      hipLaunchKernelGGL((k_tb_plan<kTbMinCopies>), dim3(gp), dim3(kBlock), 0, ctx->stream, A, par);
      hipLaunchKernelGGL((k_tb_sched<false>), gs, bs, lds_s, ctx->stream, A, par);
    }
    hipLaunchKernelGGL(k_tb_items, dim3((A.ntiles + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, A);
    if (ctx->tb.kernel == 1) hipLaunchKernelGGL((k_tbv_solve<120>), dim3(waves), dim3(64), 0, ctx->stream, A, ctx->tb.d_vtile, ctx->tb.d_vstream, ctx->tb.d_vgroups, ctx->tb.d_vexps, par);
    else if (ctx->tb.T == 64) hipLaunchKernelGGL((k_tb_solve_q<64>), dim3(waves), dim3(64), 0, ctx->stream, A, par);
    else if (ctx->tb.T == 96) hipLaunchKernelGGL((k_tb_solve_q<96>), dim3(waves), dim3(64), 0, ctx->stream, A, par);
    else if (ctx->tb.T == 120) hipLaunchKernelGGL((k_tb_solve_q<120>), dim3(waves), dim3(64), 0, ctx->stream, A, par);
    else hipLaunchKernelGGL((k_tb_solve_q<128>), dim3(waves), dim3(64), 0, ctx->stream, A, par);
  }
  hipLaunchKernelGGL(k_tb_stats, dim3(1), dim3(1024), 0, ctx->stream, A);
  HIPCHK(hipGetLastError());
  return 0;
}

// What the finalize pass needs besides the engine's result -- the output slots, the weights of its tables and the plans' records
// on the device -- depends on nothing the engine computes: it is prepared and sent BEFORE the engine runs, so that tb_fields only
// enqueues kernels behind the last chunk.  (It used to fill the records, upload them from pageable memory and synchronise after
// the last chunk had been waited for, with the device idle.)  The records are written in pinned staging that lives with the batch
// state: nothing dangles when a call ends early, and no synchronisation is needed for the host's sake.
int tb_fields_upload(mnav_ctx* ctx, uint32_t n, const std::vector<PlanIn>& in, double offset)
{
  TbState& S = ctx->tb;
  if (ensure_slots(ctx, n, false, false, ctx->want_vec)) return -1;
  if (tb_fin_weights(ctx)) return -1;
  Plan* const hp = S.h_plans.get();
  float** const vecs = S.h_vecs.get();
  // The previous pass's map of unreached pairs may be used for the leading slots that the claim covers (the caller checked it)
  // and, second lock, whose arrays are the ones that pass wrote: its records are still in the staging
  uint32_t keep = std::min(S.keep_np, n);
  for (uint32_t i = 0; i < keep; ++i) {
    const Slot& s = ctx->slots[i];
    if (hp[i].dist != s.dist.get() || hp[i].pred != s.pred.get() || vecs[i] != (float*)s.vecmap) keep = i;
  }
  S.keep_np = keep;
  for (uint32_t i = 0; i < n; ++i) {
    Slot& s = ctx->slots[i];
    Plan& P = hp[i];
    memset(&P, 0, sizeof(P));
    P.planner = kPlannerDijkstra; P.V = ctx->V;
    P.row_ptr = ctx->d_row_ptr.get(); P.nbr = ctx->d_nbr.get(); P.crn_ptr = ctx->d_crn_ptr.get(); P.crn = ctx->d_crn.get(); P.blocked = ctx->d_blocked.get();
    P.dist = s.dist.get(); P.pred = s.pred.get(); P.cap = ctx->V; P.ctl = s.ctl; P.cnt = s.cnt.get();
    P.offset = offset; P.max_steps = ctx->max_steps;
    for (int k = 0; k < 3; ++k) { P.seed[k] = in[i].seed[k]; P.target[k] = in[i].target[k]; P.seed_d[k] = 0.f; P.seed_expands[k] = 1; P.target_expands[k] = 1; }
    P.seed_face = kNone;
    vecs[i] = s.vecmap;
  }
  HIPCHK(hipMemcpyAsync(ctx->d_plans, hp, sizeof(Plan) * n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->d_vecptrs, vecs, sizeof(float*) * n, hipMemcpyHostToDevice, ctx->stream));
  return 0;
}

// per-plan arrays in vertex order: the finalize pass, for calls that want V-sized outputs (tb_fields_upload has run)
int tb_fields(mnav_ctx* ctx, uint32_t n, const tb::Args& A)
{
  TbState& S = ctx->tb;
  // potential (with the reference's tentative values beyond goal_dist), predecessors and vector map of every plan, in vertex
  // order, straight from the blocked distances: one wave per (tile, 64 plans), eight tiles per workgroup, mnav_tb_finalize.h
  FinTb F{};
  F.src = S.d_fin_src; F.w = S.d_fin_w; F.ovf = S.d_fin_ovf; F.ovf_w = S.d_fin_ovf_w; F.verts = S.d_verts; F.ghost_gid = S.d_ghost_gid; F.order = S.d_fin_order;
  F.xyz = ctx->d_xyz; F.vecmaps = ctx->want_vec ? ctx->d_vecptrs : nullptr;
  F.plans = ctx->d_plans; F.res = ctx->d_res; F.mismatch = ctx->d_mismatch; F.recs = S.d_recs;
  const uint32_t groups = (S.ntiles + kFinWaves - 1u) / kFinWaves;    // a workgroup = kFinWaves consecutive tiles of the bisection order
#ifndef MNAV_FIN_PPW
#define MNAV_FIN_PPW 64u                  // plans a wave of k_tb_finalize walks; ms of the pass per 7168-plan batch at 32 / 64 / 128 / 256: 65.8 / 66.1 / 70.6 / 79.3
#endif
  static_assert(MNAV_FIN_PPW % 64u == 0u, "a wave of k_tb_finalize owns whole words of the map of unreached pairs");
  F.plans_per_wave = MNAV_FIN_PPW; F.tiles_per_xcd = (groups + 7u) / 8u; F.max_sl = S.max_sl;
  F.umap = S.umap; F.uskip = S.uskip; F.umap_stride = S.umap_stride; F.umap_prev_np = S.keep_np; F.clean_d = S.fin_reset ? 1u : 0u;
  // settled vertices: a byte per (tile, plan) summed behind the pass instead of an atomicAdd per reached pair (option tb_fin_cnt8);
  // the bytes live with the batch state from the first pass that wants them (paths-only contexts never do)
  if (opt_u32(ctx->opt.tb_fin_cnt8, 1u) != 0u && S.ntiles) {
    if (!S.cnt8) HIPCHK(S.cnt8.alloc((size_t)S.ntiles * S.cap_np + 64));
    F.cnt8 = S.cnt8; F.cnt8_stride = S.cap_np;
  }
  hipLaunchKernelGGL(k_tb_fin_plans, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, A, ctx->d_plans, F.vecmaps, S.d_recs);
  const uint32_t npg = (n + F.plans_per_wave - 1u) / F.plans_per_wave;
  const size_t lds = 4 * (size_t)fin_lds_words(S.max_sl, F.vecmaps != nullptr) * kFinWaves;
  const dim3 grid(8u * F.tiles_per_xcd * npg);
  if (S.T == 64) hipLaunchKernelGGL((k_tb_finalize<64>), grid, dim3(64 * kFinWaves), lds, ctx->stream, A, F);
  else if (S.T == 96) hipLaunchKernelGGL((k_tb_finalize<96>), grid, dim3(64 * kFinWaves), lds, ctx->stream, A, F);
  else if (S.T == 120) hipLaunchKernelGGL((k_tb_finalize<120>), grid, dim3(64 * kFinWaves), lds, ctx->stream, A, F);
  else hipLaunchKernelGGL((k_tb_finalize<128>), grid, dim3(64 * kFinWaves), lds, ctx->stream, A, F);
  if (F.cnt8) hipLaunchKernelGGL(k_tb_fin_settled, dim3((n + kBlock - 1) / kBlock, 64), dim3(kBlock), 0, ctx->stream, F.cnt8, S.ntiles, n, F.cnt8_stride, ctx->d_res);
  HIPCHK(hipGetLastError());
  return 0;
}

// Dijkstra batches through the tile-batch engine.  Returns 0, -1 (error) or 1 (cancelled).
// The clean-up of the OTHER distance buffer for the next call, launched by the entry point when the call's last download has been
// enqueued: on its own stream, which first waits for an event recorded there, so that it starts with nothing of this call left on
// the device.  Round 6 measured where it must NOT run (profiles/r06_fill_modes.txt, r06_fill_trace.txt): next to the call's own
// kernels.  Whatever kernel of the call's stream is in flight when the fill starts does not finish before the fill does -- a 5 us
// memset took 6.9 ms next to a 7.5 ms fill -- and that is the fill's DURATION, not its rate: 48 / 24 / 12 / 6 workgroups stretched
// the batch by 0 / 6 / 18 / 40 ms.  The downloads are such kernels too (profiles/sched_pass_kernel_stats.md).  So it runs at full
// width (44 GB in 7 ms at 7168 plans) under the host's copy-out of the paths and the gap the host leaves between two calls (until
// this was moved it started after the copy-out and the call's last synchronize); a call that still comes sooner waits for the
// event, which costs what cleaning at its start would.
// It is asked for (d2_wanted_np) by every call whose finalize pass does not reset D itself: paths-only calls always, finalized ones
// unless option tb_fin_keep has bit 1 (FinTb::clean_d, mnav_tb_finalize.h -- then the call marks D clean, d_clean_np, and the next
// fresh call of no more plans neither fills nor swaps).  The second buffer is allocated by the first call that asks (tb_ensure_other).
int tb_clean_other(mnav_ctx* ctx)
{
  TbState& S = ctx->tb;
  if (!S.D2 || !S.fill_stream || S.d2_wanted_np == 0u || S.d2_clean) return 0;
  const uint32_t n = S.d2_wanted_np;
  S.d2_wanted_np = 0u;
  const size_t n16 = (4 * (size_t)S.S * n + 15) / 16;
  const uint32_t g = (uint32_t)std::max<size_t>(std::min<size_t>((n16 + kBlock - 1) / kBlock, 256 * 32), 1);
  HIPCHK(hipEventRecord(S.call_done, ctx->stream));
  HIPCHK(hipStreamWaitEvent(S.fill_stream, S.call_done, 0));
  hipLaunchKernelGGL(k_tb_fill, dim3(g), dim3(kBlock), 0, S.fill_stream, (u32x4*)S.D2.get(), n16, kTbInfBits);
  HIPCHK(hipEventRecord(S.fill_done, S.fill_stream));
  S.d2_clean = true; S.d2_clean_np = n;
  return 0;
}

// warm: the n plans do not start afresh but from their rewound resident fields (k_tb_warm, mnav_tb_warm.h) -- device arrays in
// the order of `in`: rewind levels, the potentials to read, counters (zeroed here).  Everything after the start state is the same.
struct TbWarmIn { const uint32_t* d_level; const float* const* d_dist; ReplanCnt* d_cnt; };

int run_dijkstra_tb(mnav_ctx* ctx, uint32_t n, const std::vector<PlanIn>& in, double offset, const TbWarmIn* warm = nullptr)
{
  TbState& S = ctx->tb;
  // what the caller vouches for (the claim is good for this dispatch only) and what the option allows
  const uint32_t claim_np = S.claim_np; const bool claim_vec = S.claim_vec;
  S.claim_np = 0;
  const uint32_t keep_opt = opt_u32(ctx->opt.tb_fin_keep, 1u);       // (default: the skipped stores; the reset pays in memory, not in time -- DESIGN.md section 4)
  if (tb_build(ctx)) return -1;
  if (tb_weights(ctx)) return -1;
  if (n > 65535u) { ctx->err = "tile-batch engine: more than 65535 plans in one batch"; return -1; }
  const bool grown = n > S.cap_np;                                    // (new buffers: no map, nothing clean)
  if (tb_ensure_batch(ctx, n)) return -1;
  // D is clean for was_clean plans: the mark is taken down here and put up again behind the finalize launch, so that every early
  // return leaves none
  const uint32_t was_clean = S.d_clean_np;
  S.d_clean_np = 0; S.fin_stats = false; S.filled_at_start = false;
  S.fin_reset = (keep_opt & 2u) != 0u && !ctx->lazy_paths;
  S.keep_np = ((keep_opt & 1u) && !warm && !grown && !ctx->lazy_paths && claim_vec == ctx->want_vec) ? std::min(claim_np, n) : 0u;
  if (ensure_plan_tables(ctx, n)) return -1;
  if (ensure_paths(ctx, n)) return -1;
  if (!ctx->d_mismatch) HIPCHK(ctx->d_mismatch.alloc(4));
  std::vector<uint32_t> seeds(n), targets(n);
  for (uint32_t i = 0; i < n; ++i) { seeds[i] = in[i].seed[0]; targets[i] = in[i].target[0]; }
  HIPCHK(hipMemcpyAsync(S.seed, seeds.data(), 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(S.target, targets.data(), 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_res, 0, sizeof(PlanResult) * n, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_mismatch, 0, 4, ctx->stream));
  if (!ctx->lazy_paths && tb_fields_upload(ctx, n, in, offset)) return -1;   // (V-sized outputs wanted: everything the finalize pass needs from the host, now)
  tb::Args A{};
  A.tiles = S.d_tiles; A.stream = S.d_stream; A.exps = S.d_exps; A.D = S.D; A.pend = S.pend; A.pflag = S.pflag; A.nblk = (n + 63u) / 64u; A.NP = n; A.ntiles = S.ntiles;
  A.bucket = S.bucket; A.bcnt = S.bcnt; A.items = S.items; A.ctl = S.ctl; A.wstat = S.wstat; A.wstat_slots = kTbStatSlots;
  A.marr[0] = S.marr[0]; A.marr[1] = S.marr[1]; A.mcarry = S.mcarry;
  A.thr = S.thr; A.bnd = S.bnd; A.seed = S.seed; A.target = S.target; A.vaddr = S.d_vaddr; A.vert_tile = S.d_vert_tile;
  A.offset = offset;
  // Solve kernel and band.  k_tbv_solve (distances in registers, mnav_tbv.h) takes whole waves per tile.  A plan's front crosses
  // ~sqrt(tiles) tiles per iteration, so a tile sees about 0.85 n / sqrt(tiles) plans per iteration and band of 2 tile widths
  // (measured: 63 at C2 = 7168 plans on 9 260 tiles, 11 at C4 = 4096 plans on 92 600 tiles); a wider band puts more plans on a
  // tile per iteration at the price of more activations.  Measured round 6 (engine ms per batch, k_tb_solve_q band 2 /
  // k_tbv_solve band 2 / band 4; density = n / sqrt(tiles)): 1M mesh 128 plans (density 1.3) 49 / 55 / 53, 512 (5.3) 64 / 72 / 67,
  // 2048 (21) 100 / 86 / 83, 7168 (74) 194 / 124 / 133; 10M mesh 4096 plans (13.5) 1524 / 1292 / 1180 (band 6: 1176).
  const bool v_fits = S.T == 120 && S.max_nh <= kTbvGhostRows;        // (its register window holds 120 owned rows and 64 ghosts)
  const double density = (double)n / std::sqrt((double)std::max(S.ntiles, 1u));
  S.kernel = (v_fits && density >= 8.0) ? 1 : 0;
  if (opt_set(ctx->opt.tb_kernel)) S.kernel = (opt_u32(ctx->opt.tb_kernel, 0u) == 1u && v_fits) ? 1 : 0;
  A.item_plans = S.kernel == 1 ? 64u : kTbItemPlans;
  // the schedule pass reduces the carried minima per workgroup in LDS while the plans' words fit there (mnav_tb.h)
  A.sched_lds = (tb_sched_lds_fits(n) && !(opt_set(ctx->opt.tb_sched_lds) && !opt_on(ctx->opt.tb_sched_lds))) ? 1u : 0u;
  A.min_copies = A.sched_lds ? kTbMinCopiesLds : kTbMinCopies;
  A.sweep_seq = opt_u32(ctx->opt.tb_sweep_seq, 1u) != 0u ? 1u : 0u;
  {
    const float band_mult = (S.kernel == 1 && density < 40.0) ? 4.0f : S.band_mult;
    float band = (ctx->delta_auto / 3.0f) * std::sqrt((float)S.T) * band_mult;   // potential across one tile
    if (opt_set(ctx->opt.tb_band_mult)) band = (ctx->delta_auto / 3.0f) * std::sqrt((float)S.T) * (float)ctx->opt.tb_band_mult;
    if (ctx->tile_band_user > 0.f) band = ctx->tile_band_user;
    A.band = band;
  }
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  if (!warm) {
    bool prefilled = was_clean >= n;                                  // the previous call's finalize pass left D clean: no fill, no swap
    if (!prefilled) {
      if (S.D2 && S.d2_clean && S.d2_clean_np >= n) {                 // a clean buffer was prepared behind the previous call
        std::swap(S.D, S.D2); A.D = S.D;
        HIPCHK(hipStreamWaitEvent(ctx->stream, S.fill_done, 0));
        prefilled = true;
      }
      S.d2_clean = false;
    }
    S.filled_at_start = !prefilled;
    if (!prefilled && tb_fill(ctx, S.D, 4 * (size_t)S.S * n, kTbInfBits)) return -1;
    if (tb_fill(ctx, S.pend, 4 * (size_t)S.ntiles * n, kTbInfBits)) return -1;
  }
  // (a warm start writes every word of its slices and pending words itself: it neither waits for a prepared clean buffer nor
  // uses it up -- the buffer stays clean for the next fresh batch)
  HIPCHK(hipMemsetAsync(S.pflag, 0, (size_t)(S.ntiles ? S.ntiles : 1) * ((n + 63u) / 64u) + 64u, ctx->stream));
  if (tb_fill(ctx, S.marr[0], 4 * (size_t)n, kTbInfBits)) return -1;
  if (tb_fill(ctx, S.marr[1], 4 * (size_t)n, kTbInfBits)) return -1;
  if (tb_fill(ctx, S.mcarry, 4 * (size_t)kTbMinCopies * n, kTbInfBits)) return -1;
  HIPCHK(hipMemsetAsync(S.ctl, 0, sizeof(tb::Ctl), ctx->stream));
  HIPCHK(hipMemsetAsync(S.wstat, 0, 32 * (size_t)kTbStatSlots, ctx->stream));
  HIPCHK(hipMemsetAsync(S.bcnt, 0, 4 * (size_t)(S.ntiles ? S.ntiles : 1), ctx->stream));
  if (warm) {
    if (!S.warm_ev[0]) for (auto& e : S.warm_ev) HIPCHK(hipEventCreate(e.out()));
    HIPCHK(hipMemsetAsync(warm->d_cnt, 0, sizeof(ReplanCnt) * (size_t)n, ctx->stream));
    TbWarm Wm{};
    Wm.level = warm->d_level; Wm.dist = warm->d_dist; Wm.cnt = warm->d_cnt;
    Wm.verts = S.d_verts; Wm.ghost_gid = S.d_ghost_gid; Wm.order = S.d_fin_order; Wm.T = S.T;
    const size_t groups = (size_t)std::max(S.ntiles, 1u) * ((n + 63u) / 64u);
    if (groups >= (1ull << 31)) { ctx->err = "tile-batch engine: warm start beyond 2^31 workgroups"; return -1; }
    HIPCHK(hipEventRecord(S.warm_ev[0], ctx->stream));
    if (S.ntiles) hipLaunchKernelGGL(k_tb_warm, dim3((uint32_t)groups), dim3(kWarmBlock), 0, ctx->stream, A, Wm);
    HIPCHK(hipEventRecord(S.warm_ev[1], ctx->stream));
  } else
  hipLaunchKernelGGL(k_tb_seed, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, A);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
  // (the other buffer -- the previous call's distances, superseded the moment this call began -- is cleaned for the NEXT call behind
  // the last kernel of this one: tb_clean_other)
  // -- unless this call's finalize pass resets the buffer it works in (FinTb::clean_d): then there is no other buffer to prepare
  if (!S.fin_reset && tb_ensure_other(ctx)) return -1;
  if (!warm || !S.d2_clean) S.d2_wanted_np = (S.D2 && !S.fin_reset) ? n : 0u;

  int ncu = 256;
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device);
  uint32_t per_cu = (uint32_t)((160u * 1024u) / (S.T * 256u + kTbQStride * 4u));   // LDS: T x 256 bytes + staging per wave, 160 KB per CU
  if (S.kernel == 1) per_cu = 8u;                                      // k_tbv_solve: 256 VGPRs per wave, two waves per SIMD, no LDS
  if (opt_set(ctx->opt.tb_waves_per_cu)) S.waves_per_cu = (int)ctx->opt.tb_waves_per_cu;
  if (S.waves_per_cu > 0) per_cu = (uint32_t)S.waves_per_cu;
  const uint32_t waves = std::min(per_cu * (uint32_t)ncu, kTbStatSlots);   // (a wave beyond the statistics' slots would go uncounted)
  const int chunk = S.iters_per_replay & ~1;
  // graph of `chunk` iterations, re-captured when the kernel arguments change
  int gi = 0;                                                         // graph slot: the one captured with these arguments, else the older one
  for (int k = 0; k < 2; ++k) if (S.graph[k] && memcmp(&S.graph_args[k], &A, sizeof(A)) == 0) gi = k + 2;
  if (ctx->use_graph && gi < 2) {
    gi = (S.graph[0] && S.graph_args[0].D != A.D) ? 1 : 0;
    S.graph[gi].reset();
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    const int rc = tb_launch_iterations(ctx, A, chunk, waves);
    const hipError_t e = hipStreamEndCapture(ctx->stream, &g);
    if (rc != 0 || e != hipSuccess) { ctx->err = "graph capture failed"; return -1; }
    HIPCHK(hipGraphInstantiate(S.graph[gi].out(), g, nullptr, nullptr, 0));
    (void)hipGraphDestroy(g);
    memcpy(&S.graph_args[gi], &A, sizeof(A));
  } else gi -= 2;
  int rc = 0;
  uint32_t iters = 0;
  const auto t_start = std::chrono::steady_clock::now();
  HIPCHK(hipEventRecord(ctx->evc[0], ctx->stream));
  for (;;) {
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() > ctx->max_wall_s) {
      ctx->err = "tile-batch iterations exceeded the wall-clock guard"; return -1;
    }
    if (ctx->use_graph) HIPCHK(hipGraphLaunch(S.graph[gi], ctx->stream));
    else if (tb_launch_iterations(ctx, A, chunk, waves)) return -1;
    iters += (uint32_t)chunk;
    HIPCHK(hipMemcpyAsync(S.h_ctl, S.ctl, sizeof(tb::Ctl), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (S.h_ctl->err) { ctx->err = "tile-batch engine: sweep cap hit"; return -1; }
    if (S.h_ctl->n_cand[0] == 0u) break;                             // the chunk ends on odd parity: its pending count is counter 0
    if (ctx->cancel.load(std::memory_order_relaxed)) { rc = 1; break; }
    if (iters > ctx->max_steps) { ctx->err = "tile-batch engine: iteration cap hit"; return -1; }
  }
  HIPCHK(hipEventRecord(ctx->evc[1], ctx->stream));
  if (rc == 0 && !ctx->lazy_paths) {
    // V-sized outputs wanted (potential, predecessors, vector map): the finalize pass of the tile engines derives the
    // reference's exact cut-off semantics and predecessors straight from the blocked distances (k_tb_finalize)
    if (warm) HIPCHK(hipEventRecord(S.warm_ev[2], ctx->stream));
    if (tb_fields(ctx, n, A)) return -1;
    if (warm) HIPCHK(hipEventRecord(S.warm_ev[3], ctx->stream));
    // the pass is enqueued: behind it every word of the first n plans is +inf again (the reached slices reset, the others never
    // written), and so is what was clean beyond them.  A warm start of more plans than were clean wrote its slices only.
    if (S.fin_reset) S.d_clean_np = warm ? (n <= was_clean ? was_clean : 0u) : std::max(n, was_clean);
    S.fin_stats = true; S.fin_np = n;
  }
  HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
  HIPCHK(hipEventSynchronize(ctx->evc[1]));
  ctx->ms_chunks = ev_ms(ctx->evc[0], ctx->evc[1]);
  S.last = *S.h_ctl;
  if (warm && rc == 0) {
    HIPCHK(hipEventSynchronize(S.warm_ev[3]));
    S.ms_warm = ev_ms(S.warm_ev[0], S.warm_ev[1]); S.ms_warm_fin = ev_ms(S.warm_ev[2], S.warm_ev[3]);
  }
  ctx->stats.launches = 1;                                           // one engine run per batch (iterations: stats.steps)
  ctx->tb_args = A; ctx->tb_args_valid = (rc == 0);
  if (opt_on(ctx->opt.trace))
    fprintf(stderr, "[mnav] tile-batch: %u iterations, %llu activations (%.1f per item), %llu items, %.2f sweeps per item, %llu wakes, carried minima %s\n", S.h_ctl->iters,
            S.h_ctl->acts, S.h_ctl->items ? (double)S.h_ctl->acts / S.h_ctl->items : 0.0, S.h_ctl->items,
            S.h_ctl->items ? (double)S.h_ctl->sweeps / S.h_ctl->items : 0.0, S.h_ctl->wakes, A.sched_lds ? "reduced in LDS" : "in global memory");
  return rc;
}
