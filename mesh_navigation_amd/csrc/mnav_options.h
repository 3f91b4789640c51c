// mnav_options.h -- the tuning / debug options of a context.  The process environment is read ONCE, by mnav_create
// (MNAV_<NAME IN CAPITALS>); afterwards only mnav_set_option changes an option: no getenv on any plan path, a variable that
// appears in the environment of a running mbf_mesh_nav node changes nothing.  Unset (NaN) = the built-in default of the place
// that reads it.  Included by mnav.hip; not a stand-alone header.
#pragma once

#define MNAV_OPTION_LIST(X)                                                                                                              \
  X(verbose)             /* 1: one line per engine build / asynchronous call on stderr */                                                 \
  X(trace)               /* 1: host-side trace points on stderr */                                                                        \
  X(no_graph)            /* 1: launch the step / round kernels one by one instead of replaying hipGraphs (profilers that cannot see into graphs) */ \
  X(debug_chunk)         /* step launches per host look when no_graph is set: rounded up to a multiple of 6 (the kernels rotate their control blocks by launch % 6 and every chunk starts at 0); below 1: the default, 96; the result does not depend on it */ \
  X(dijkstra_engine)     /* 0 tile rounds, 1 band steps, 3 auto, 5 tile-batch, 6 asynchronous tiles */                            \
  X(blocks_per_plan)     /* band steps: workgroups per plan */                                                                            \
  X(tile_blocks)         /* tile rounds: workgroups per plan */                                                                           \
  X(cvp_wide)            /* 0 / 1: never / always the wide CVP step kernel (default: batches from 32 plans) */                            \
  X(wide_waves)          /* wide CVP kernel: resident waves */                                                                            \
  X(cvp_groups)          /* wide CVP kernel: groups of plans stepped on their own streams (default by batch size, <= 4) */                \
  X(max_steps) X(max_wall_s)                                                                                                             \
  X(cvp_verify)          /* 0: skip the verification sweeps after a CVP plan */                                                           \
  X(key_walk_max) X(descend_walk_max)   /* cascade-tree walk bounds (tests) */                                                            \
  X(tile_size)           /* LDS tiles, read at mnav_upload_mesh */                                                                        \
  X(lazy_paths)          /* 0: always run the finalize pass */                                                                            \
  X(tile_band) X(rounds_band_mult)                                                                                                       \
  X(tb_tile)             /* tile-batch engine: rows per tile, read when its streams are built */                                          \
  X(tb_no_prefill) X(tb_band_mult) X(tb_waves_per_cu)                                                                                    \
  X(tb_kernel)           /* tile-batch solve: 0 = k_tb_solve_q (16 plans per quarter of a wave, distances in LDS), 1 = k_tbv_solve (64 plans per wave, distances in registers); default: by the expected plans per tile */ \
  X(tb_sched_lds)        /* tile-batch schedule pass: 0 = every carried value goes to the global copies of the plans' minima; default: a workgroup reduces its tiles' values in LDS first, while the batch's plans fit there */ \
  X(tb_sweep_seq)        /* tile-batch solve, k_tbv_solve: 1 (default) = the sweeps of an item run the orders its lanes voted for first, most votes first, then rotate on; 0 = the most voted order, then the rotation through the other three (the result does not depend on it) */ \
  X(tb_fin_keep)         /* tile-batch finalize pass, what it keeps for the next call: bit 0 = it skips the stores of a (tile, plan) that is unreached again, bit 1 = it resets the distance buffer itself instead of a fill (default 1: measured, the reset gains no time and frees the second distance buffer; 3: both; 0: neither; the result does not depend on it) */ \
  X(tb_fin_cnt8)         /* tile-batch finalize pass, settled vertices per plan: 1 (default, measured: DESIGN.md section 3.1) = a byte per (tile, plan), stored 64 at a time and summed by a kernel behind the pass (one byte per pair of device memory, from the first such pass on); 0 = one atomicAdd per reached pair; the result does not depend on it */ \
  X(async_wg_per_cu) X(async_wg_per_plan) X(async_max_s)                                                                          \
  X(async_band_mult)     /* band of the asynchronous engine in tile widths of potential (default 4; <= 0: no bands) */                         \
  X(async_max_batch)     /* auto: batches of up to this many plans take the asynchronous engine */                                      \
  X(async_ring_cap)      /* ticket slots of the asynchronous engine (default 16 per tile and plan; tests force the overflow path) */       \
  X(nbhd_lds_cap)        /* neighbourhood layers: members per centre in LDS (default 128, 32..512; tests force the spill path) */ \
  X(replan_log_cap)      /* replan: entries of the change log (default V; tests force the overflow) */                                    \
  X(replan_fresh_below)  /* replan: plan afresh when the smallest rewind level / old cut of the batch lies below this fraction (default 0.25; 0: never) */ \
  X(replan_each_fresh_share) /* per-plan replan: plan the whole call afresh when more than this share of its plans is FRESH (default 0.004, measured; 1: never) */ \
  X(replan_repair_engine) /* replan: what finishes the repaired plans -- 0 the tile rounds, 5 the tile-batch engine started from the rewound fields (k_tb_warm); unset: by replan_warm_min_plans */ \
  X(replan_warm_min_plans) /* replan, replan_repair_engine unset: the tile-batch warm start from this many repaired plans on (default 299, measured: DESIGN.md section 3.14) */ \
  X(fleet_scratch_mb)    /* fleet walks: MiB of scratch rows per chunk of robots (default 256; the result does not depend on it) */ \
  X(dispatch_max_mb)     /* fleet dispatch: MiB of device matrix (5 bytes per pair, 9 for an assignment) a call may take (default 4096) */ \
  X(dispatch_max_rounds) /* fleet assign: auction rounds after which the call gives up (default 4194304) */ \
  X(dispatch_tail_bidders) /* fleet assign: rounds with at most this many unassigned bidders run in the single-workgroup tail kernel (default 16, measured, at most 8192; 0: never; the result does not depend on it) */ \
  X(traffic_combine)     /* fleet traffic: 1 = a wave whose contributors all end on one vertex issues one add for them, 0 = one add per lane (default 0, measured: within 1 % either way; the counts do not depend on it) */ \
  X(timed_traffic_max_mb) /* timed fleet traffic: MiB of cells and holders (8 bytes per vertex and window; 20 with the tentative arrays of a fleet schedule) a call may take (default 2048; 0 refuses every call) */ \
  X(timed_peak_blocks)   /* timed fleet traffic: blocks of the peak pass, which stride over the vertices (default 2048; the result does not depend on it; tests force the strided path) */ \
  X(schedule_chunk_rounds) /* fleet schedule: rounds enqueued between two looks of the host at the control record (default 8; the result does not depend on it) */ \
  X(schedule_clean_fill) /* fleet schedule: 1 = the tentative arrays are filled between the rounds, 0 = the claimants clean their own words in the commit pass (default 0; the result does not depend on it) */ \
  X(separation_cell_scale) /* fleet rollout: side of the separation check's grid cells in radii, 1 .. 4 (default 2; the result does not depend on it) */ \
  X(separation_max_tests) /* fleet rollout: a check whose pair pass would perform more distance tests than this is skipped (default 2^32, provisional: DESIGN.md section 3.20) */ \
  X(ring_early_exit)     /* fleet rollout rings: 1 = a round of the doubling whose earlier rounds already cover the robots held returns at once, 0 (default, measured: DESIGN.md section 3.22) = every round runs (the result does not depend on it) */

struct Options {
#define X(name) double name = NAN;
  MNAV_OPTION_LIST(X)
#undef X
  struct Desc { const char* name; double Options::*field; };
  static const Desc* table(size_t* n)
  {
    static const Desc t[] = {
#define X(name) { #name, &Options::name },
      MNAV_OPTION_LIST(X)
#undef X
    };
    *n = sizeof(t) / sizeof(t[0]);
    return t;
  }
  double* find(const char* name)
  {
    size_t n; const Desc* t = table(&n);
    for (size_t i = 0; i < n; ++i) if (!strcmp(t[i].name, name)) return &(this->*t[i].field);
    return nullptr;
  }
  // MNAV_<NAME> for every option; dijkstra_engine also takes the engines' names
  void from_environment()
  {
    size_t n; const Desc* t = table(&n);
    for (size_t i = 0; i < n; ++i) {
      std::string var = "MNAV_";
      for (const char* c = t[i].name; *c; ++c) var += (char)toupper((unsigned char)*c);
      const char* e = getenv(var.c_str());
      if (!e || !*e) continue;
      double v = atof(e);
      if (!strcmp(t[i].name, "dijkstra_engine")) {
        v = !strcmp(e, "tiled") ? 0 : !strcmp(e, "band") ? 1 : !strcmp(e, "tile_batch") ? 5 : !strcmp(e, "async") ? 6
          : (e[0] >= '0' && e[0] <= '9') ? atof(e) : 3;
      }
      this->*t[i].field = v;
    }
  }
};
static inline bool opt_set(double v) { return v == v; }
static inline uint32_t opt_u32(double v, uint32_t dflt) { return v == v ? (uint32_t)(v < 0.0 ? 0.0 : v) : dflt; }
static inline bool opt_on(double v) { return v == v && v != 0.0; }
