// mnav_graph_capi.h -- the C ABI of the resident layer graph (include/mnav.h: mnav_map_*) over the kernels of mnav_graph.h.
// Included by mnav.hip inside its extern "C" block, after mnav_obstacle_capi.h (mnav_map_obstacle runs the obstacle pass).
//
// List lengths: every stage reads its 16 bytes of counters back before the next one is launched (one stream synchronisation
// per stage), so every launch has its exact grid and no kernel is started on an empty list.
#pragma once

static int map_fail(mnav_ctx* ctx, const char* what) { ctx->err = what; return -1; }

// the node pass of `rule` over slot L: counters into S.h_cnt, the outgoing list into `ids`
extern "C++" {
template <class Rule>
static int map_node_pass(mnav_ctx* ctx, mnav_ctx::Layer& L, const Rule& rule, uint32_t* ids)
{
  using namespace mnav_map;
  State& S = ctx->map;
  const uint32_t V = ctx->V, nblk = blocks(V) ? blocks(V) : 1, fresh = L.ready ? 0u : 1u;
  hipLaunchKernelGGL(k_node_count<Rule>, dim3(nblk), dim3(kChgBlock), 0, ctx->stream, V, rule, fresh, L.cost, L.lethal, S.blk, nblk);
  hipLaunchKernelGGL(k_node_scan, dim3(1), dim3(kChgBlock), 0, ctx->stream, nblk, S.blk, S.cnt);
  hipLaunchKernelGGL(k_node_emit<Rule>, dim3(nblk), dim3(kChgBlock), 0, ctx->stream, V, rule, fresh, L.cost, L.lethal, S.blk, nblk, ids);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(S.h_cnt, S.cnt, sizeof(uint32_t) * kCounters, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}
}  // extern "C++"

int mnav_map_configure(mnav_ctx* ctx, uint32_t n_nodes, const mnav_map_node* nodes, uint32_t default_layer, double edge_cost_factor,
                       const uint8_t* invalid)
{
  using namespace mnav_map;
  if (!ctx) return -1;
  ctx->err.clear();
  if (!ctx->have_mesh) return map_fail(ctx, "mnav_upload_mesh has not been called");
  if (!n_nodes || n_nodes > kMaxLayers || !nodes) return map_fail(ctx, "layer graph: 1..64 nodes");
  static_assert(MNAV_NODE_INPUT == 0 && MNAV_NODE_INFLATION == 1 && MNAV_NODE_COMBINE_MAX == 2 && MNAV_NODE_COMBINE_AVG == 3, "node kinds");
  // everything is checked before anything is allocated or replaced: a refused call leaves the previous configuration
  int decl[kMaxLayers];
  for (uint32_t k = 0; k < kMaxLayers; ++k) decl[k] = -1;
  for (uint32_t i = 0; i < n_nodes; ++i) {
    const mnav_map_node& N = nodes[i];
    if (N.layer >= kMaxLayers) return map_fail(ctx, "layer graph: slot out of range (64 layers)");
    if (decl[N.layer] >= 0) return map_fail(ctx, "layer graph: a slot is listed twice");
    decl[N.layer] = (int)i;
    if (N.kind > MNAV_NODE_COMBINE_AVG) return map_fail(ctx, "layer graph: unknown node kind");
    const bool ok = N.kind == MNAV_NODE_INPUT ? N.n_inputs == 0 : N.kind == MNAV_NODE_INFLATION ? N.n_inputs == 1 : (N.n_inputs >= 1 && N.n_inputs <= kMaxInputs);
    if (!ok) return map_fail(ctx, "layer graph: wrong number of inputs for the node kind (input 0, inflation 1, combination 1..8)");
  }
  for (uint32_t i = 0; i < n_nodes; ++i)
    for (uint32_t k = 0; k < nodes[i].n_inputs; ++k)
      if (nodes[i].inputs[k] >= kMaxLayers || decl[nodes[i].inputs[k]] < 0) return map_fail(ctx, "layer graph: an input is not a node");
  if (default_layer >= kMaxLayers || decl[default_layer] < 0) return map_fail(ctx, "layer graph: the default layer is not a node");
  // dependency order: repeatedly the first declared node whose inputs are all placed (inputs before users)
  std::vector<uint32_t> order;
  bool placed[kMaxLayers] = {};
  while (order.size() < n_nodes) {
    bool any = false;
    for (uint32_t i = 0; i < n_nodes; ++i) {
      if (placed[nodes[i].layer]) continue;
      bool ready = true;
      for (uint32_t k = 0; k < nodes[i].n_inputs; ++k) ready = ready && placed[nodes[i].inputs[k]];
      if (!ready) continue;
      placed[nodes[i].layer] = true; order.push_back(i); any = true;
    }
    if (!any) return map_fail(ctx, "layer graph: cycle");
  }
  if (hipSetDevice(ctx->device) != hipSuccess) return map_fail(ctx, "hipSetDevice failed");
  const uint32_t V = ctx->V;
  const size_t Vn = V ? V : 1, nblk = blocks(V) ? blocks(V) : 1;
  State S;
  for (uint32_t k = 0; k < kMaxLayers; ++k) S.pos[k] = -1;
  std::vector<CombTab> tabs;
  for (uint32_t i : order) {
    const mnav_map_node& N = nodes[i];
    if (layer_slot(ctx, N.layer, N.kind == MNAV_NODE_INFLATION)) return -1;
    Node n;
    n.layer = N.layer; n.kind = N.kind; n.n_in = N.n_inputs;
    for (uint32_t k = 0; k < N.n_inputs; ++k) { n.in[k] = N.inputs[k]; n.w[k] = N.weights[k]; }
    n.p[0] = N.inflation_radius; n.p[1] = N.inscribed_radius; n.p[2] = N.inscribed_value; n.p[3] = N.lethal_value; n.p[4] = N.cost_scaling_factor;
    HIPCHK(n.ids.alloc(sizeof(uint32_t) * Vn));
    if (N.kind >= MNAV_NODE_COMBINE_MAX) {
      CombTab T{};
      for (uint32_t k = 0; k < N.n_inputs; ++k) {                    // (inputs come first in `order`: their slots exist)
        T.cost[k] = ctx->layers[N.inputs[k]].cost; T.lethal[k] = ctx->layers[N.inputs[k]].lethal; T.w[k] = N.weights[k];
      }
      T.n = N.n_inputs; T.mode = N.kind == MNAV_NODE_COMBINE_MAX ? 0 : 1;
      n.tab = (int)tabs.size();
      tabs.push_back(T);
    }
    S.pos[N.layer] = (int)S.order.size();
    S.order.push_back(std::move(n));
  }
  S.default_layer = default_layer; S.edge_cost_factor = edge_cost_factor;
  S.have_invalid = invalid != nullptr;
  HIPCHK(S.d_tabs.alloc(sizeof(CombTab) * (tabs.size() ? tabs.size() : 1)));
  if (!tabs.empty()) HIPCHK(hipMemcpyAsync(S.d_tabs, tabs.data(), sizeof(CombTab) * tabs.size(), hipMemcpyHostToDevice, ctx->stream));
  if (invalid) {
    S.h_invalid.assign(invalid, invalid + V);
    HIPCHK(S.d_invalid.alloc(Vn));
    HIPCHK(hipMemcpyAsync(S.d_invalid, S.h_invalid.data(), V, hipMemcpyHostToDevice, ctx->stream));
  }
  if (alloc_group(S.stamp, Vn, S.blk, sizeof(uint32_t) * 4 * nblk, S.cnt, sizeof(uint32_t) * kCounters, S.vals, sizeof(float) * Vn) != hipSuccess ||
      S.h_cnt.alloc(sizeof(uint32_t) * kCounters) != hipSuccess) return map_fail(ctx, "layer graph: out of memory");
  HIPCHK(hipMemsetAsync(S.stamp, 0, Vn, ctx->stream));
  for (auto& e : S.ev) HIPCHK(hipEventCreate(e.out()));
  HIPCHK(hipStreamSynchronize(ctx->stream));                         // `tabs` goes out of scope
  S.configured = true;
  ctx->map = std::move(S);
  return 0;
}

// readMap's layer part (mesh_map.cpp:427-448): derived nodes in order, copyVertexCostsFromDefaultLayer, computeEdgeWeights
int mnav_map_compute(mnav_ctx* ctx)
{
  using namespace mnav_map;
  if (!ctx) return -1;
  ctx->err.clear();
  State& S = ctx->map;
  if (!S.configured) return map_fail(ctx, "no layer graph (mnav_map_configure first)");
  if (hipSetDevice(ctx->device) != hipSuccess) return map_fail(ctx, "hipSetDevice failed");
  for (const Node& n : S.order)
    if (n.kind == MNAV_NODE_INPUT && !ctx->layers[n.layer].ready) return map_fail(ctx, "layer graph: an input layer is not resident");
  S.computed = false; S.stale = true;                                // until the whole pass went through
  ctx->rp.all = true;                                                // whole arrays replaced: a replan plans afresh, also after a failure half way
  const uint32_t V = ctx->V, gb = (V + kBlock - 1) / kBlock ? (V + kBlock - 1) / kBlock : 1;
  for (const Node& n : S.order) {
    if (n.kind == MNAV_NODE_INFLATION) {
      if (layer_inflation_impl(ctx, n.layer, n.in[0], n.p[0], n.p[1], n.p[2], n.p[3], n.p[4], nullptr, S.d_invalid, nullptr)) return -1;
    } else if (n.kind != MNAV_NODE_INPUT) {
      mnav_ctx::Layer& L = ctx->layers[n.layer];
      hipLaunchKernelGGL(k_comb_slot, dim3(gb), dim3(kBlock), 0, ctx->stream, V, S.d_tabs + n.tab, L.cost, L.lethal);
      HIPCHK(hipGetLastError());
      layer_commit_plain(L);
    }
  }
  if (ensure_edge_distances(ctx)) return -1;
  HIPCHK(ctx->d_cost.upload(ctx->stream, nullptr, V));
  HIPCHK(hipMemcpyAsync(ctx->d_cost, ctx->layers[S.default_layer].cost, sizeof(float) * V, hipMemcpyDeviceToDevice, ctx->stream));
  if (edge_weight_pass(ctx, S.edge_cost_factor, S.have_invalid ? S.h_invalid.data() : nullptr, nullptr, nullptr)) return -1;
  S.computed = true; S.stale = false;
  return 0;
}

static int map_update_ready(mnav_ctx* ctx, uint32_t layer, bool want_input)
{
  using namespace mnav_map;
  const State& S = ctx->map;
  if (!S.configured) return map_fail(ctx, "no layer graph (mnav_map_configure first)");
  if (S.stale) return map_fail(ctx, "layer graph: stale after a failed call (mnav_map_compute first)");
  if (!S.computed) return map_fail(ctx, "layer graph: not computed yet (mnav_map_compute first)");
  if (layer >= kMaxLayers || S.pos[layer] < 0) return map_fail(ctx, "layer graph: the layer is not a node");
  if (want_input && S.order[S.pos[layer]].kind != MNAV_NODE_INPUT) return map_fail(ctx, "layer graph: the layer is a derived node (owned by the graph)");
  if (hipSetDevice(ctx->device) != hipSuccess) return map_fail(ctx, "hipSetDevice failed");
  return 0;
}

// Steps 2 and 3 of an update: node `src` of S.order has its outgoing list set; the dependents follow in order, then the
// default layer's list D reaches the resident vertex costs, the edge weights and the host mirror.
static int map_propagate(mnav_ctx* ctx, uint32_t src, uint32_t* changed_out, uint32_t* n_changed)
{
  using namespace mnav_map;
  State& S = ctx->map;
  const uint32_t V = ctx->V;
  S.waves = S.recombined = S.default_changed = S.edges_reweighted = 0; S.ms_wave = 0.f;
  for (uint32_t i = 0; i < S.order.size(); ++i) if (i != src) { S.order[i].out = nullptr; S.order[i].n_out = S.order[i].flipped = 0; }
  for (uint32_t i = src + 1; i < S.order.size(); ++i) {
    Node& n = S.order[i];
    if (n.kind == MNAV_NODE_INPUT) continue;
    mnav_ctx::Layer& L = ctx->layers[n.layer];
    if (n.kind == MNAV_NODE_INFLATION) {
      const Node& in = S.order[S.pos[n.in[0]]];
      if (!in.n_out || !in.flipped) continue;                        // no lethal flag of the input changed: the wave would repeat itself
      const Diff d{ n.ids, S.blk, S.cnt, S.h_cnt };
      if (layer_inflation_impl(ctx, n.layer, n.in[0], n.p[0], n.p[1], n.p[2], n.p[3], n.p[4], nullptr, S.d_invalid, &d)) return -1;
      ++S.waves; S.ms_wave += ctx->infl_ms;
    } else {
      bool any = false;
      for (uint32_t k = 0; k < n.n_in; ++k) {
        const Node& in = S.order[S.pos[n.in[k]]];
        if (!in.n_out) continue;
        hipLaunchKernelGGL(k_stamp_ids, dim3((in.n_out + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, in.n_out, in.out, (uint8_t)1, S.stamp);
        any = true;
      }
      if (!any) continue;
      const int rc = map_node_pass(ctx, L, CombRule{ S.d_tabs + n.tab, S.stamp }, n.ids);
      for (uint32_t k = 0; k < n.n_in; ++k) {                        // the stamp is cleared by the lists that set it
        const Node& in = S.order[S.pos[n.in[k]]];
        if (in.n_out) hipLaunchKernelGGL(k_stamp_ids, dim3((in.n_out + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, in.n_out, in.out, (uint8_t)0, S.stamp);
      }
      HIPCHK(hipGetLastError());
      if (rc) return -1;
      S.recombined += S.h_cnt[kActive];
    }
    n.out = n.ids; n.n_out = S.h_cnt[kOut]; n.flipped = S.h_cnt[kFlipped];
  }
  // D: the default layer's outgoing list
  const Node& dn = S.order[S.pos[S.default_layer]];
  const uint32_t nd = dn.n_out;
  S.default_changed = nd;
  if (nd) {
    const uint32_t g = (nd + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_gather_costs, dim3(g), dim3(kBlock), 0, ctx->stream, nd, dn.out, ctx->layers[dn.layer].cost, S.vals);
    hipLaunchKernelGGL(k_scatter_costs, dim3(g), dim3(kBlock), 0, ctx->stream, nd, dn.out, S.vals, ctx->d_cost);
    if (ctx->edge_cost_factor != 0.0)                               // "Edge costs are only affected by vertex costs if layer_factor is not 0" (:568-572)
      hipLaunchKernelGGL(k_update_edge_weights, dim3((8 * (size_t)nd + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, nd, dn.out, ctx->d_row_ptr,
                         ctx->d_nbr_u, ctx->d_nbr_e, ctx->d_edge_dist, ctx->d_cost, ctx->edge_cost_factor, ctx->d_w);
    HIPCHK(hipGetLastError());
    replan_log_vertices(ctx, dn.out, nd);                           // D is what a replan has to look at (mnav_replan.h)
    S.h_ids.resize(nd); S.h_vals.resize(nd);
    HIPCHK(hipMemcpyAsync(S.h_ids.data(), dn.out, sizeof(uint32_t) * nd, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(S.h_vals.data(), S.vals, sizeof(float) * nd, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipEventRecord(S.ev[1], ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (uint32_t i = 0; i < nd; ++i) {
    const uint32_t v = S.h_ids[i];
    if (v >= V) return map_fail(ctx, "layer graph: change list out of range");
    ctx->h_cost[v] = S.h_vals[i];
    if (ctx->edge_cost_factor != 0.0) S.edges_reweighted += ctx->h_row_ptr[v + 1] - ctx->h_row_ptr[v];
  }
  if (nd) ctx->nbr_valid = ctx->crn_valid = false;                  // the cost-limit folded copies are rebuilt on the next plan
  if (changed_out && nd) memcpy(changed_out, S.h_ids.data(), sizeof(uint32_t) * nd);
  if (n_changed) *n_changed = nd;
  S.ms_total = ev_ms(S.ev[0], S.ev[1]);
  return 0;
}

// the caller's ids, checked, as an ascending duplicate-free list (of a run of equal ids the last one counts, as in a loop over them)
static int map_sorted_ids(mnav_ctx* ctx, uint32_t n, const uint32_t* vertex_ids, std::vector<uint32_t>& ids, std::vector<uint32_t>& last)
{
  if (n && !vertex_ids) return map_fail(ctx, "null id array");
  for (uint32_t i = 0; i < n; ++i) if (vertex_ids[i] >= ctx->V) return map_fail(ctx, "vertex id out of range");
  std::vector<uint32_t> idx(n);
  for (uint32_t i = 0; i < n; ++i) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return vertex_ids[a] != vertex_ids[b] ? vertex_ids[a] < vertex_ids[b] : a < b; });
  ids.clear(); last.clear();
  for (uint32_t k = 0; k < n; ++k) {
    if (k + 1 < n && vertex_ids[idx[k + 1]] == vertex_ids[idx[k]]) continue;
    ids.push_back(vertex_ids[idx[k]]); last.push_back(idx[k]);
  }
  return 0;
}

static int map_finish(mnav_ctx* ctx, int rc)
{
  if (rc) { ctx->map.stale = true; ctx->rp.all = true; (void)hipStreamSynchronize(ctx->stream); }   // (how far the update got is unknown: a replan plans afresh)
  return rc;
}

int mnav_map_layer_changed(mnav_ctx* ctx, uint32_t layer, uint32_t n, const uint32_t* vertex_ids, uint32_t* changed_out, uint32_t* n_changed)
{
  using namespace mnav_map;
  if (!ctx) return -1;
  ctx->err.clear();
  if (map_update_ready(ctx, layer, true)) return -1;
  State& S = ctx->map;
  if (!ctx->layers[layer].ready) return map_fail(ctx, "layer graph: the input layer is not resident");
  std::vector<uint32_t> ids, last;
  if (map_sorted_ids(ctx, n, vertex_ids, ids, last)) return -1;
  Node& src = S.order[S.pos[layer]];
  HIPCHK(hipEventRecord(S.ev[0], ctx->stream));
  const uint32_t m = (uint32_t)ids.size();
  if (m) HIPCHK(hipMemcpyAsync(src.ids, ids.data(), sizeof(uint32_t) * m, hipMemcpyHostToDevice, ctx->stream));
  src.out = src.ids; src.n_out = m; src.flipped = m;                 // which flags flipped is the writer's knowledge: assume some did
  const int rc = map_propagate(ctx, (uint32_t)S.pos[layer], changed_out, n_changed);   // (its synchronisations cover `ids`)
  return map_finish(ctx, rc);
}

int mnav_map_update_layer(mnav_ctx* ctx, uint32_t layer, uint32_t n, const uint32_t* vertex_ids, const float* costs, const uint8_t* lethal,
                          uint32_t* changed_out, uint32_t* n_changed)
{
  using namespace mnav_map;
  if (!ctx) return -1;
  ctx->err.clear();
  if (map_update_ready(ctx, layer, true)) return -1;
  State& S = ctx->map;
  mnav_ctx::Layer& L = ctx->layers[layer];
  if (!L.ready) return map_fail(ctx, "layer graph: the input layer is not resident");
  if (n && !costs) return map_fail(ctx, "null cost array");
  std::vector<uint32_t> ids, last;
  if (map_sorted_ids(ctx, n, vertex_ids, ids, last)) return -1;     // ids >= V: refused before anything is written
  const uint32_t m = (uint32_t)ids.size();
  std::vector<float> vals(m);
  std::vector<uint8_t> flags(lethal ? m : 0);
  for (uint32_t k = 0; k < m; ++k) { vals[k] = costs[last[k]]; if (lethal) flags[k] = lethal[last[k]] ? 1 : 0; }
  if (m > S.up_cap) {
    S.up_cap = 0;
    if (alloc_group(S.up_vals, sizeof(float) * m, S.up_flags, m) != hipSuccess) return map_fail(ctx, "layer graph: out of memory");
    S.up_cap = m;
  }
  Node& src = S.order[S.pos[layer]];
  HIPCHK(hipEventRecord(S.ev[0], ctx->stream));
  uint32_t flipped = 0;
  if (m) {
    int rc = 0;
    if (hipMemcpyAsync(src.ids, ids.data(), sizeof(uint32_t) * m, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(S.up_vals, vals.data(), sizeof(float) * m, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        (lethal && hipMemcpyAsync(S.up_flags, flags.data(), m, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) ||
        hipMemsetAsync(S.cnt + kScatterFlipped, 0, sizeof(uint32_t), ctx->stream) != hipSuccess) rc = -1;
    if (rc == 0) {
      hipLaunchKernelGGL(k_scatter_layer, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, m, src.ids, S.up_vals,
                         lethal ? S.up_flags.get() : (const uint8_t*)nullptr, L.cost, L.lethal, S.cnt);
      if (hipGetLastError() != hipSuccess ||
          hipMemcpyAsync(S.h_cnt, S.cnt, sizeof(uint32_t) * kCounters, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = -1;
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) rc = -1;   // the host vectors stay alive until here
    if (rc) { ctx->err = "layer graph: layer update failed"; return map_finish(ctx, rc); }
    flipped = S.h_cnt[kScatterFlipped];
  }
  src.out = src.ids; src.n_out = m; src.flipped = flipped;          // the list is the given ids, as in the harness's ArrayLayer::update
  return map_finish(ctx, map_propagate(ctx, (uint32_t)S.pos[layer], changed_out, n_changed));
}

int mnav_map_obstacle(mnav_ctx* ctx, uint32_t layer, uint32_t n_points, const void* points, uint32_t point_step, const float* sensor_to_map,
                      const float* down_axis, double robot_height, double max_obstacle_dist, uint32_t* changed_out, uint32_t* n_changed)
{
  using namespace mnav_map;
  if (!ctx) return -1;
  ctx->err.clear();
  if (map_update_ready(ctx, layer, true)) return -1;
  if (obstacle_check_args(ctx, n_points, points, point_step, down_axis)) return -1;   // (the graph stays usable)
  State& S = ctx->map;
  HIPCHK(hipEventRecord(S.ev[0], ctx->stream));
  uint32_t nc = 0;
  // the obstacle pass leaves its list (the vertices whose flag flipped) in the change-list scratch: it stays there
  if (mnav_layer_obstacle(ctx, layer, n_points, points, point_step, sensor_to_map, down_axis, robot_height, max_obstacle_dist, nullptr, &nc, nullptr))
    return map_finish(ctx, -1);
  Node& src = S.order[S.pos[layer]];
  src.out = ctx->chg.ids; src.n_out = nc; src.flipped = nc;
  return map_finish(ctx, map_propagate(ctx, (uint32_t)S.pos[layer], changed_out, n_changed));
}

int mnav_map_stats(const mnav_ctx* ctx, uint32_t* waves, uint32_t* recombined, uint32_t* default_changed, uint32_t* edges_reweighted,
                   float* ms_total, float* ms_wave)
{
  if (!ctx) return -1;
  const mnav_map::State& S = ctx->map;
  if (waves) *waves = S.waves;
  if (recombined) *recombined = S.recombined;
  if (default_changed) *default_changed = S.default_changed;
  if (edges_reweighted) *edges_reweighted = S.edges_reweighted;
  if (ms_total) *ms_total = S.ms_total;
  if (ms_wave) *ms_wave = S.ms_wave;
  return 0;
}
