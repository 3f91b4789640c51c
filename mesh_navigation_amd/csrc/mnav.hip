// mnav.hip -- MI355X (gfx950) wavefront planner: HIP kernels + the C ABI of include/mnav.h.
//
// Hot path replaced (reference file:line):
//   DijkstraMeshPlanner::dijkstra       dijkstra_mesh_planner/src/dijkstra_mesh_planner.cpp:217-398
//   DijkstraMeshPlanner::computeVectorMap                                            :189-209
//   CVPMeshPlanner::waveFrontPropagation cvp_mesh_planner/src/cvp_mesh_planner.cpp:651-918
//   CVPMeshPlanner::waveFrontUpdate                                                  :369-556
//   CVPMeshPlanner::computeVectorMap                                                 :204-239
//   MeshMap::computeEdgeWeights          mesh_map/src/mesh_map.cpp:517-561
//
// Design: the priority-queue loops become distance bands settled by a gather
// rule iterated to its fixed point (mnav_eval.h).  One step = one launch of k_step over the
// current work list of every plan in the batch; steps are enqueued back-to-back from a
// hipGraph with no host round trip, all loop control (band advance, goal_dist arming,
// termination) is recomputed by every workgroup from the previous step's counters.
// Memory-bound irregular gather work: no MFMA, coalescing via CSR rows + 24-byte corner
// records, wave-aggregated atomics for the work lists.
//
// This file never computes a plan on the CPU: every entry point fails when no GPU is usable.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>
#include <unordered_map>
#include <unistd.h>

#include "../../include/mnav.h"
#include "mnav_buf.h"
#include "mnav_build.h"
#include "mnav_eval.h"
#include "mnav_options.h"
#include "mnav_resident.h"

using namespace mnav;

namespace {

// Pointers that reach a kernel through a struct in memory are generic to the compiler: it emits
// flat_load + s_waitcnt vmcnt(0) lgkmcnt(0) around every LDS access.  Device-memory arrays are
// therefore re-typed as address_space(1) before use (global_load, waits only on vmcnt).
#define MNAV_GLOBAL __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ MNAV_GLOBAL T* as_global(T* p) { return (MNAV_GLOBAL T*)p; }
template <class T>
__device__ __forceinline__ MNAV_GLOBAL T* as_global(const GPtr<T>& p) { return (MNAV_GLOBAL T*)p.p; }
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));   // one Nbr {u, w bits}
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));   // 16-byte copy unit

constexpr int kBlock = 256;   // streaming kernels (init, vector map, input preparation)
constexpr int kChunk = 96;  // step launches per graph replay; multiple of 6 (slot parities)

#include "mnav_band.h"

#include "mnav_tiles.h"

#include "mnav_shard.h"   // kernels of the sharded single plan (k_shard_*)

#include "mnav_finalize.h"

#include "mnav_plan_kernels.h"

#include "mnav_map_kernels.h"

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
}  // namespace
#include "mnav_tb.h"
#include "mnav_tb_finalize.h"
#include "mnav_tbv.h"
#include "mnav_walk.h"
#include "mnav_obstacle.h"   // obstacle layer: LBVH build, ray cast (mnav_obs::); the change list of mnav_changelist.h (mnav_chg::)
#include "mnav_nbhd.h"       // height-difference / roughness / ridge layers: neighbourhood visits (mnav_nb::)
#include "mnav_clearance.h"  // clearance / border layers: normal ray casts over the obstacle BVH, border test (mnav_clr::)
#include "mnav_locate.h"     // pose lookup: point LBVH over the vertices, exact nearest vertex, containing face (mnav_loc::)
#include "mnav_follow.h"     // vector-field follower: one controller tick for a batch of robots over the resident fields (mnav_fol::)
#include "mnav_rollout.h"    // device rollouts: many controller ticks per call over resident robot state (mnav_rol::)
#include "mnav_fleet_rollout.h"   // fleet rollouts: a departure tick per robot and the separation check between robots (mnav_frol::)
#include "mnav_fleet_yield.h"     // ... in which robots yield: the right-of-way rule inside the check's pair pass, held robots without a tick (mnav_frol::)
#include "mnav_fleet_ring.h"      // ... and learn why they are held: the wait-for analysis behind the pair pass, the release of rings (mnav_frol::)
#include "mnav_sample.h"     // sampled rollouts: K candidate controls per robot, scored on the potential and picked on the device (mnav_smp::)
#include "mnav_replan.h"     // replan on a resident potential: rewind level from the change log, rewind with the tiles' wake-up words (k_replan_*)
#include "mnav_replan_each.h"  // the per-plan replan: class of every plan, ordered lists, compacted records (k_replan_classify, k_replan_gather)
#include "mnav_tb_warm.h"    // warm start of the tile-batch engine from rewound fields: every slice and pending word of a sub-batch (k_tb_warm)
#include "mnav_graph.h"      // resident layer graph: node passes with change lists, id-list union, combination into a slot (mnav_map::)

// One back-tracking job: the plan's resident vector map and the two ends of the walk.
struct WalkJob { const float* vecmap; float seed[3]; uint32_t seed_face; float target[3]; uint32_t target_face; };

// CVPMeshPlanner's back-tracking (cvp_mesh_planner.cpp:920-951) on the resident vector map: one wave per plan.  The loop
// is a dependent chain (each step needs the position the previous one produced), so all 64 lanes walk in lockstep on the
// same data (uniform loads, uniform branches) and divide only the scan of searchNeighbourFaces' face list, which lives in
// LDS.  ctl[2*j] = walk status, ctl[2*j+1] = entries written (walk order, target first).
__global__ __launch_bounds__(64) void k_backtrack(WalkMesh M, WalkInflation L, const WalkJob* __restrict__ jobs, double step_width, uint32_t cap,
                                                  float* __restrict__ pos_out, uint32_t* __restrict__ face_out, int32_t* __restrict__ ctl)
{
  __shared__ uint32_t list[kWalkScratchWords];
  const uint32_t j = blockIdx.x;
  const WalkJob J = jobs[j];
  if (!J.vecmap) { if (threadIdx.x == 0) { ctl[2 * j] = 0; ctl[2 * j + 1] = 0; } return; }   // no plan behind this row
  WalkField Fd;
  Fd.vecmap = J.vecmap;
  for (int k = 0; k < 3; ++k) Fd.seed_vs[k] = M.faces[3 * (size_t)J.seed_face + k];
  uint32_t n = 0;
  const int st = walk_backtrack(M, Fd, L, w3(J.seed[0], J.seed[1], J.seed[2]), J.seed_face, w3(J.target[0], J.target[1], J.target[2]), J.target_face,
                                step_width, cap, pos_out + 3 * (size_t)cap * j, face_out + (size_t)cap * j, &n, list);
  ctl[2 * j] = st; ctl[2 * j + 1] = (int32_t)n;
}
#include "mnav_fleet.h"      // fleet paths and walks: many robots per resident field (mnav_fleet::; after the locate and follow headers, and after WalkJob)
#include "mnav_plans.h"      // fleet plans: makePlan's pose lists and costs over those paths and walks (mnav_fleet::, mnav_pose.h)
#include "mnav_dispatch.h"   // fleet dispatch: the robot-to-goal cost matrix over the resident fields and the auction on it (mnav_dispatch::)
#include "mnav_traffic.h"    // fleet traffic: path-occupancy counts over the resident fields and the congestion cost layer (mnav_traffic::)
#include "mnav_timed.h"      // timed fleet traffic: occupancy per (vertex, time window), holders and the yield report (mnav_timed::)
#include "mnav_schedule.h"   // fleet schedule: conflict-free departure delays on the timed cells, round by round (mnav_schedule::)
namespace {

struct Slot {
  DevBuf<float> dist, dirn, vecmap;
  DevBuf<PopKey> tkey;
  DevBuf<uint32_t> pred, cutf, stamp, dirty, list0, list1;
  DevBuf<uint32_t> wlist0, wlist1, wstamp;
  Ctl* ctl = nullptr;                  // (into d_ctl_pool)
  DevBuf<Cnt> cnt;
  bool cvp_ready = false, band_ready = false;
  // tiled engine
  DevBuf<uint32_t> tpend0, tpend1;
  DevBuf<float> tlast;
  TCtl* tctl = nullptr;                // (into d_tctl_pool)
  DevBuf<TCnt> tcnt;
  bool tile_ready = false;
};

}  // namespace

struct mnav_ctx {
  int device = 0;
  Stream stream;
  std::string err;
  std::atomic<int> cancel{ 0 };
  DevBuf<uint32_t> d_cancel;               // the same flag in device memory: long-running kernels poll it (agent-scope load)
  PinnedBuf<uint32_t> h_one;               // pinned source word (1) for the copy mnav_cancel issues on its own stream
  Stream cancel_stream;
  // host copies needed for seeding
  uint32_t V = 0, F = 0, E = 0;
  std::vector<float> h_xyz, h_cost;
  std::vector<uint32_t> h_row_ptr, h_nbr_u;   // gather CSR (host copy): the tile-batch engine builds its streams from it on first use
  TbState tb; tb::Args tb_args{};             // tile-batch SSSP engine (mnav_tb.h); arguments of the last batch
  bool tb_args_valid = false;                 // ... which still describe live device memory (last tile-batch call succeeded, nothing freed since)
  bool mesh_since_outputs = false;            // mnav_upload_mesh ran since the last plan call began its outputs: mnav_last_engine names no engine
  bool want_vec = false;               // parameter of the RUNNING call: it asked for vector maps (lazy 12 B/vertex/plan).  What the outputs
                                       // left behind hold is the record's to say (ctx->res)
  bool resident_vecmap = false;        // mnav_set_resident_outputs: always compute the vector map, leave it on the device
  Resident res;                        // what the last plan call left on the device (mnav_resident.h): every reader of resident outputs asks it
  std::vector<uint32_t> h_faces;
  std::vector<uint32_t> h_vf_ptr, h_vf;    // getFacesOfVertex rows (host copy; uploaded on the first device back-tracking call)
  DevBuf<uint32_t> d_faces, d_vf_ptr, d_vf; bool walk_mesh_valid = false;
  DevBuf<float> d_walk_pos; DevBuf<uint32_t> d_walk_face; size_t walk_cap = 0;   // k_backtrack outputs: rows of `cap` entries
  Event ev_link[2];                        // stream links of the asynchronous shard calls (caller's stream <-> ours)
  DevBuf<WalkJob> d_walk_jobs; DevBuf<int32_t> d_walk_ctl; uint32_t walk_jobs_cap = 0;
  std::vector<uint8_t> h_invalid;
  bool have_mesh = false, have_costs = false, have_normals = false;
  // device mesh
  DevBuf<uint32_t> d_row_ptr, d_nbr_u, d_nbr_e, d_crn_ptr, d_edge_vtx;
  DevBuf<CornerIdx> d_crn_idx;
  DevBuf<uint32_t> d_crn_walk;                                      // HostTopology::crn_walk (inflation vector field)
  DevBuf<float> d_xyz, d_nrm, d_cost, d_w, d_edge_dist;
  DevBuf<uint8_t> d_invalid;
  // materialised per cost_limit
  DevBuf<Nbr> d_nbr; double nbr_limit = NAN; bool nbr_valid = false;
  DevBuf<Corner> d_crn; DevBuf<uint8_t> d_blocked; double crn_limit = NAN; bool crn_valid = false;
  FaceCirculation circ;                                            // caller-supplied getFacesOfVertex rows (optional)
  DevBuf<uint32_t> d_verify_any; uint32_t verify_sweeps_used = 0;
  bool cvp_verify = true;                                          // k_cvp_verify after every CVP plan (MNAV_CVP_VERIFY=0 to skip)
  int walk_max = kKeyWalkMax, descend_max = kDescendWalkMax;       // cascade-tree walk bounds (MNAV_KEY_WALK_MAX / MNAV_DESCEND_WALK_MAX: tests)
  // plans
  std::vector<Slot> slots;
  DevBuf<Plan> d_plans; uint32_t plans_cap = 0;
  DevBuf<PlanResult> d_res; PinnedBuf<PlanResult> h_res;
  DevBuf<float*> d_vecptrs;
  DevBuf<uint32_t> d_paths; size_t paths_words = 0; uint32_t path_stride = 0;   // n plans x path_stride vertex ids
  DevBuf<uint32_t> d_over; DevBuf<unsigned long long> d_over_off; DevBuf<uint32_t> d_over_cap;   // exact rows of the paths that did not fit
  DevBuf<uint32_t> d_pack; PinnedBuf<uint32_t> h_pack; DevBuf<uint32_t> d_pack_meta; size_t pack_words = 0, h_pack_words = 0, pack_meta_n = 0;   // packed paths (device, pinned host), offsets + lengths
  PinnedBuf<uint32_t> h_mism;   // the fixed-point check's counter, downloaded with the results
  PinnedBuf<Ctl> h_ctl;       // 2 per plan
  uint32_t infl_exact_bands = 0;   // bands of the last inflation wave that went through the exact band routine (k_exact_band)
  DevBuf<float> d_seed_pos; uint32_t seed_pos_cap = 1;
  std::map<uint64_t, GraphExec> graphs;
  // tiled SSSP engine
  int dij_engine = 3;          // 0 tiled rounds, 1 band steps, 3 auto, 5 tile-batch, 6 asynchronous tiles (2: the per-plan persistent kernel, retired round 5)
  int last_engine = 0;
  bool lazy_paths = false;      // parameter of the RUNNING call: it only wants vertex paths, k_path_lazy instead of k_dij_finalize + k_finish
                                // (whether the outputs left behind are paths-only: ctx->res)
  bool allow_lazy_paths = true; // MNAV_LAZY_PATHS=0: always finalize (predecessors / tentative values for everybody)
  uint32_t max_steps = 1u << 20;   // per plan; set from the mesh size at upload (a wavefront needs O(diameter) steps)
  double max_wall_s = 120.0;   // host-side guard: a plan that takes longer is abandoned with an error
  uint32_t tile_size = 512;    // 4 workgroups of the tile kernels per CU (36 KB LDS each)
  float rounds_band_mult = 4.0f;   // the round engine (latency) prefers wide bands
  float tile_band_user = 0.f, tile_band_auto = 1.f;
  DevBuf<uint32_t> d_t_rptr;
  HostTiles tiles_meta;        // only the small per-tile vectors are kept (vert_tile, sizes)
  DevBuf<uint32_t> d_t_vptr, d_t_verts, d_t_hptr, d_t_halo_verts, d_t_halo_tile, d_t_eptr, d_t_src, d_vert_tile, d_mismatch;
  DevBuf<uint16_t> d_t_rowptr, d_t_col;
  DevBuf<float> d_t_tw; bool tw_valid = false; uint32_t t_nnz = 0;
  // sharded single plan (mnav_shard_*)
  struct Shard {
    bool ready = false, active = false, finalized = false;   // finalized: slot 0 holds the predecessors of the last sharded plan (mnav_shard_walk)
    uint32_t rank = 0, world = 1, t_lo = 0, t_hi = 0, n_iface = 0, rounds_per_exchange = 8, j = 0;
    uint32_t seed = 0, target = 0; double offset = 0.3; uint32_t goal_tie1 = 0;
    DevBuf<uint32_t> d_iface_vert, d_wake_ptr, d_wake_tile, d_changed, d_minpend;
    DevBuf<uint8_t> d_iface_owner;
    std::vector<uint32_t> iface_vert;
    bool partition = false; DevBuf<uint8_t> d_owned;                 // mnav_shard_setup_partition
    DevBuf<uint32_t> d_walk; uint32_t walk_cap = 0;                  // mnav_shard_walk
    std::map<std::array<uint64_t, 3>, GraphExec> graphs;             // captured exchange sequences (shard_replay)
  } shard;
  double edge_cost_factor = 0.0;                                   // factor of the resident edge weights (mnav_update_costs)
  // layers computed / kept on the device (mnav_layer_*)
  struct Layer { DevBuf<float> cost; DevBuf<uint8_t> lethal; DevBuf<float> dist, vec; DevBuf<uint8_t> vstate;   // vstate: 3 x V (two state arrays + the accumulate flags)
                 bool ready = false, have_vec = false;
                 double inflation_radius = 0, inscribed_radius = 0, inscribed_value = 0, lethal_value = 0; };   // InflationLayer config (vectorAt reads it)
  std::vector<Layer> layers;
  DevBuf<Corner> d_crn_infl; bool crn_infl_valid = false;          // corners over the edge distances (inflation wave)
  DevBuf<uint8_t> d_infl_mask, d_zero_u8;
  DevBuf<float> d_infl_keyd;
  mnav_obs::Bvh obs;                                               // obstacle layer: BVH built by the first mnav_layer_obstacle after an upload
  mnav_nb::State nbhd;                                             // neighbourhood layers: counters, spill lists and scratch of the last call
  mnav_clr::State clr;                                             // clearance / border layers: cached clearance (first clearance call after an upload)
  mnav_loc::State loc;                                             // pose lookup: vertex index built by the first mnav_locate after an upload
  mnav_fol::Staging stage;                                         // follower and rollout: the per-robot inputs of the running call, the two work lists
  mnav_fol::State fol;                                             // vector-field follower: outputs and counters of the last mnav_follow_batch
  mnav_fleet::State fleet;                                         // fleet paths / walks: buffers and statistics of the last mnav_fleet_* call
  mnav_dispatch::State dispatch;                                   // fleet dispatch: the matrix, the auction's state and the statistics of the last mnav_fleet_costs / _assign
  mnav_traffic::State traffic;                                     // fleet traffic: the V counts, their total and the statistics of the last mnav_fleet_traffic
  mnav_timed::State timed;                                         // timed fleet traffic: the V x B cells and holders, the peaks and the statistics of the last mnav_fleet_timed_traffic
  mnav_schedule::State schedule;                                   // fleet schedule: the V x B tentative counts and holders, the control record and the statistics of the last mnav_fleet_schedule
  mnav_fleet::PlanState plans;                                     // fleet plans: counts, costs, id / length scratch and packed poses of the last call
  DevBuf<float> d_fnrm; bool have_face_normals = false;            // MeshMap::faceNormals() (mnav_upload_face_normals): F x 3, gone with the mesh
  mnav_rol::Dev rol;                                               // device rollouts, both entry points: the rest of the resident robot state, goals, counter rows, trace
  mnav_frol::State frol;                                           // fleet rollout: start ticks, the separation check's table, records, rows and check rows, its event pairs
  struct RolloutRecord { mnav_rol::Stats rol; mnav_frol::SepStats sep; mnav_frol::YldStats yld; mnav_frol::RingStats ring; };   // what one rollout entry point's *_stats tell of its last call
  RolloutRecord rol_rec, frol_rec, yld_rec, ring_rec;              // mnav_follow_rollout, mnav_fleet_rollout, mnav_fleet_rollout_yield, mnav_fleet_rollout_rings: kept apart
  mnav_frol::YldState yld;                                         // yielding fleet rollout: hold flags, priorities, yield rows and check rows, the pair passes' event pairs
  mnav_frol::RingState ring;                                       // wait-for analysis: blockers, the doubling's buffers, marks, ring rows and check rows, its event pairs
  mnav_smp::Dev smp; mnav_smp::Stats smp_rec;                      // sampled rollouts: the uploaded robots, the rows' pot / lethal / cmd0 / score, the picks; the last call's record
  mnav_chg::Scratch chg;                                           // obstacle / clearance / border layers: change list and counters of the last call
  mnav_map::State map;                                             // resident layer graph (mnav_map_*): nodes, tables, change lists of the last update
  uint32_t infl_steps = 0, infl_bands = 0; uint64_t infl_evals = 0; float infl_ms = 0.f, infl_ms_wave = 0.f;   // last inflation wave
  DevBuf<TilePlan> d_tplans; uint32_t tplans_cap = 0;
  PinnedBuf<TCtl> h_tctl;
  size_t tile_lds = 0, fin_lds = 0;
  bool use_graph = true;
  DevBuf<uint32_t> d_wide_prefix; DevBuf<WideSched> d_wide_sched; uint32_t wide_cap = 0;   // k_cvp_ctl -> k_step_wide
  DevBuf<float> d_vec3;                                              // mnav_vector_at after a paths-only batch
  uint32_t wide_groups = 1; Stream stream_g[kWideGroupsMax]; Event ev_fork[kWideGroupsMax];   // CVP batches in groups on their own streams ([0] unused / fork event)
  uint32_t cvp_wide_min_batch = 32;                                  // CVP batches of at least this many plans run k_step_wide
  float delta_user = 0.f, delta_auto = 0.f;
  Options opt;                                                       // mnav_options.h: read from the environment once, by mnav_create
  uint32_t max_steps_auto = 1u << 20;
  DevBuf<uint32_t> d_ring; uint32_t ring_cap = 0; size_t ring_words = 0; PinnedBuf<AsyncCtl> h_actl; DevBuf<uint32_t> d_parked; size_t parked_words = 0;   // asynchronous tile engine: ticket ring, pinned copy of its control words
  // replan on the resident potentials (mnav_replan_dijkstra_batch)
  struct Replan {
    // change log: vertices whose cost, blocked status or incident edge weights may have changed since the last Dijkstra call.
    // Every writer knows its count on the host, so the length lives there; `all`: a writer replaced whole arrays, or the log ran over
    DevBuf<uint32_t> log; uint32_t len = 0; bool all = false;
    // (the recorded Dijkstra call itself, its slot map and what can be rewound: ctx->res)
    int each_engines = 0;            // mnav_last_engine after mnav_replan_dijkstra_each repaired per plan: 256 + (128: tile rounds ran) + (512: the REPAIRED plans ran warm on the
                                     // tile-batch engine, 1024: with k_tbv_solve) + (engine of the FRESH sub-batch, 127: none)
    // the warm repair on the tile-batch engine (k_tb_warm): its device arrays in sub-batch order and the statistics of the last
    // replan call of either kind (mnav_replan_warm_stats).  live: no other planner call has run since a warm repair
    struct Warm {
      DevBuf<uint32_t> d_level; DevBuf<const float*> d_dist; DevBuf<ReplanCnt> d_cnt; uint32_t cap = 0;
      uint32_t plans = 0, kernel = 0, iters = 0, fallback = 0; uint64_t woken = 0, words = 0; bool live = false;
      float ms_warm = 0.f, ms_engine = 0.f, ms_finalize = 0.f;
    } warm;
    DevBuf<uint32_t> d_level, d_old_target; DevBuf<float> d_cut; DevBuf<ReplanCnt> d_cnt; uint32_t cap = 0;
    Event ev[5]; bool have_ev = false;
    // statistics of the last replan call (mnav_replan_stats)
    uint32_t reason = 0, stat_log_len = 0, tiles_woken = 0, rounds = 0; uint64_t kept = 0, rewound = 0; std::vector<float> levels;
    float ms_level = 0.f, ms_rewind = 0.f, ms_rounds = 0.f, ms_finalize = 0.f;
    // mnav_replan_dijkstra_each: classes, lists and the compacted tables of the plans that go on; its statistics
    struct Each {
      DevBuf<uint8_t> d_cls; DevBuf<float> d_ratio; DevBuf<uint32_t> d_lists, d_counts, d_level;
      DevBuf<Plan> d_plans; DevBuf<TilePlan> d_tplans; DevBuf<float*> d_vecptrs; DevBuf<ReplanCnt> d_cnt; DevBuf<TCtl> d_tctl; DevBuf<PlanResult> d_res;
      uint32_t cap = 0;
      Event ev[7]; bool have_ev = false;
      uint32_t reason = 0, whole_fresh = 0, log_len = 0, counts[3] = { 0, 0, 0 }, tiles_woken = 0, rounds = 0; int fresh_engine = -1;
      uint64_t kept = 0, rewound = 0; std::vector<uint8_t> cls; std::vector<float> levels;
      float ms_classify = 0.f, ms_rewind = 0.f, ms_rounds = 0.f, ms_finalize = 0.f, ms_fresh = 0.f;
    } each;
  } rp;
  mnav_stats stats{};
  uint64_t algo_bytes = 0;
  Event ev[8];
  Event evc[2];                // bracket one graph replay (chunk of step/round launches)
  double ms_chunks = 0.0;      // sum of the bracketed chunk durations of the last call
  DevBuf<Ctl> d_ctl_pool; uint32_t ctl_pool_cap = 0;         // contiguous control blocks: one D2H copy per chunk
  DevBuf<TCtl> d_tctl_pool; uint32_t tctl_pool_cap = 0;
};

namespace {

#define MTRACE(msg) do { if (opt_on(ctx->opt.trace)) { fprintf(stderr, "[mnav] %9.3f ms %s:%d %s\n", 1e-3 * (double)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(), __func__, __LINE__, msg); fflush(stderr); } } while (0)
#define HIPCHK(call)                                                                               \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess) {                                                                        \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e_) + " (" __FILE_NAME__ ":" + std::to_string(__LINE__) + ")"; \
      return -1;                                                                                   \
    }                                                                                              \
  } while (0)

float ev_ms(hipEvent_t a, hipEvent_t b);

void drop_graphs(mnav_ctx* ctx)
{
  ctx->graphs.clear();
  ctx->shard.graphs.clear();
}

// the options that are mirrored in context fields (everything else is read from ctx->opt where it is used)
void apply_options(mnav_ctx* ctx)
{
  const Options& o = ctx->opt;
  ctx->use_graph = !opt_on(o.no_graph);
  if (opt_set(o.dijkstra_engine)) { const int e = (int)o.dijkstra_engine; ctx->dij_engine = (e == 0 || e == 1 || e == 5 || e == 6) ? e : 3; }
  else ctx->dij_engine = 3;                                           // unset (NaN): the built-in default, auto
  ctx->max_steps = opt_u32(o.max_steps, ctx->max_steps_auto);
  ctx->max_wall_s = opt_set(o.max_wall_s) ? o.max_wall_s : 120.0;
  ctx->cvp_verify = !opt_set(o.cvp_verify) || o.cvp_verify != 0.0;
  ctx->walk_max = opt_set(o.key_walk_max) ? (int)o.key_walk_max : kKeyWalkMax;
  ctx->descend_max = opt_set(o.descend_walk_max) ? (int)o.descend_walk_max : kDescendWalkMax;
  ctx->allow_lazy_paths = !opt_set(o.lazy_paths) || o.lazy_paths != 0.0;
  ctx->tile_band_user = opt_set(o.tile_band) ? (float)o.tile_band : 0.f;
  ctx->rounds_band_mult = opt_set(o.rounds_band_mult) ? (float)o.rounds_band_mult : 4.0f;
}

int ensure_plan_tables(mnav_ctx* ctx, uint32_t n);

int ensure_slots(mnav_ctx* ctx, uint32_t n, bool cvp, bool band, bool vec)
{
  const size_t V = ctx->V ? ctx->V : 1;
  while (ctx->slots.size() < n) {
    Slot s;
    HIPCHK(s.dist.alloc(4 * V)); HIPCHK(s.pred.alloc(4 * V));          // 8 B per vertex and plan ...
    HIPCHK(s.cnt.alloc(4 * sizeof(Cnt)));                              // 3 rotating + sticky flags
    ctx->slots.push_back(std::move(s));
  }
  for (uint32_t i = 0; i < n; ++i) {                                   // ... the rest only for the paths that use it
    Slot& s = ctx->slots[i];
    if (band && !s.band_ready) {                                       // work lists of the band/gather steps
      HIPCHK(alloc_group(s.stamp, 4 * V, s.dirty, 4 * V, s.list0, 4 * V, s.list1, 4 * V, s.wlist0, 4 * V, s.wlist1, 4 * V, s.wstamp, 4 * V));
      s.band_ready = true;
    }
    if (vec && !s.vecmap) HIPCHK(s.vecmap.alloc(12 * V));
  }
  if (cvp)
    for (uint32_t i = 0; i < n; ++i) {
      Slot& s = ctx->slots[i];
      if (!s.cvp_ready) {
        HIPCHK(alloc_group(s.tkey, sizeof(PopKey) * V, s.dirn, 4 * V, s.cutf, 4 * V));
        s.cvp_ready = true;
      }
    }
  if (ctx->ctl_pool_cap < n) {
    HIPCHK(ctx->d_ctl_pool.alloc(2 * sizeof(Ctl) * n));
    ctx->ctl_pool_cap = n;
  }
  for (uint32_t i = 0; i < n; ++i) ctx->slots[i].ctl = ctx->d_ctl_pool + 2 * i;
  return ensure_plan_tables(ctx, n);
}

// per-plan tables shared by all engines (plan descriptors, results)
int ensure_plan_tables(mnav_ctx* ctx, uint32_t n)
{
  if (ctx->plans_cap < n) {
    ctx->d_plans.reset(); ctx->d_res.reset(); ctx->h_res.reset(); ctx->h_ctl.reset(); ctx->d_vecptrs.reset();
    drop_graphs(ctx);   // graphs captured the old d_plans pointer
    HIPCHK(ctx->d_plans.alloc(sizeof(Plan) * n));
    HIPCHK(ctx->d_res.alloc(sizeof(PlanResult) * n));
    HIPCHK(ctx->h_res.alloc(sizeof(PlanResult) * n));
    HIPCHK(ctx->h_ctl.alloc(sizeof(Ctl) * 2 * n));
    HIPCHK(ctx->d_vecptrs.alloc(sizeof(float*) * n));
    ctx->plans_cap = n;
  }
  return 0;
}

// Vertex paths of a batch: n rows of `stride` ids.  A path has ~1.4 sqrt(V) hops on a terrain, so rows of
// 16 sqrt(V) + 1024 ids hold it with a wide margin (84 MB instead of 20 GB for 5120 plans on the 1M mesh); a path
// that does not fit makes the path kernels report kPathOverflow with the full length, and only those plans are walked
// again into rows of exactly that size.
uint32_t default_path_stride(const mnav_ctx* ctx)
{
  const double s = 16.0 * std::sqrt((double)ctx->V) + 1024.0;
  return (uint32_t)std::min<double>(s, (double)(ctx->V ? ctx->V : 1));
}
int ensure_paths(mnav_ctx* ctx, uint32_t n, uint32_t stride)
{
  const size_t words = (size_t)n * (stride ? stride : 1);
  if (ctx->paths_words < words) {
    ctx->paths_words = 0;
    HIPCHK(ctx->d_paths.alloc(sizeof(uint32_t) * words));
    ctx->paths_words = words;
  }
  ctx->path_stride = stride;
  return 0;
}
int ensure_paths(mnav_ctx* ctx, uint32_t n) { return ensure_paths(ctx, n, default_path_stride(ctx)); }

uint32_t blocks_per_plan(const mnav_ctx* ctx)
{
  // the work list of a planar mesh is O(sqrt(V)) long; 8 entries per wave and round.  Measured on the 1M mesh (CVP,
  // MI355X): 500 waves per plan are as fast as 1500 for a single plan (41.8 vs 41.4 ms) and 25 % faster in a batch of
  // 128 (225 vs 178 plans/s: fewer idle waves to dispatch per step); 256 waves cost 5 % / 10 %.
  const double want = 4.0 * std::sqrt((double)ctx->V) / kGroupsPerWave;
  uint32_t g = (uint32_t)std::ceil(want);
  if (opt_set(ctx->opt.blocks_per_plan)) g = opt_u32(ctx->opt.blocks_per_plan, g);
  if (g < 4) g = 4;
  if (g > 4096) g = 4096;
  return g;
}

template <uint32_t PLANNER>
int launch_steps(mnav_ctx* ctx, uint32_t n, uint32_t G, int count, bool wide)
{
  const bool fork = wide && ctx->wide_groups > 1;
  if (fork) {                                                          // the other streams join (the capture of) the first
    HIPCHK(hipEventRecord(ctx->ev_fork[0], ctx->stream));
    for (uint32_t g = 1; g < ctx->wide_groups; ++g) HIPCHK(hipStreamWaitEvent(ctx->stream_g[g], ctx->ev_fork[0], 0));
  }
  for (int j = 0; j < count; ++j) {
    if (wide) {
      // per group of plans: controller + shares, the wide kernel with as many waves as stay resident, and the 8-lane kernel for the
      // plans in a band cut.  The groups run on two streams (two branches of the captured graph): a step of one group is ~0.6
      // rounds of the resident waves, so where one group's last round leaves the machine half empty the other group's step fills it
      uint32_t off = 0, poff = 0;
      for (uint32_t g = 0; g < ctx->wide_groups; ++g) {
        const uint32_t ng = (n * (g + 1u)) / ctx->wide_groups - off;
        hipStream_t st = g == 0 ? ctx->stream : ctx->stream_g[g];
        if (ng) {
          hipLaunchKernelGGL(k_cvp_ctl, dim3(1), dim3(256), 0, st, ctx->d_plans + off, ng, j % 6, ctx->d_wide_prefix + poff, ctx->d_wide_sched + g);
          hipLaunchKernelGGL(k_step_wide, dim3(G), dim3(kWave), 0, st, ctx->d_plans + off, ng, j % 6, ctx->d_wide_prefix + poff, ctx->d_wide_sched + g);
          hipLaunchKernelGGL(k_step_repair, dim3(blocks_per_plan(ctx), kRepairRows), dim3(kWave), 0, st, ctx->d_plans + off, j % 6,
                             ctx->d_wide_prefix + poff + ng + 1u, ctx->d_wide_sched + g);
        }
        off += ng; poff += 2u * ng + 2u;
      }
    }
    else hipLaunchKernelGGL(k_step<PLANNER>, dim3(G, n), dim3(kWave), 0, ctx->stream, ctx->d_plans, j % 6);
  }
  if (fork) {
    for (uint32_t g = 1; g < ctx->wide_groups; ++g) {
      HIPCHK(hipEventRecord(ctx->ev_fork[g], ctx->stream_g[g]));
      HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_fork[g], 0));
    }
  }
  HIPCHK(hipGetLastError());
  return 0;
}

__global__ void k_stamp_to_host(unsigned long long* __restrict__ dst_host) { *dst_host = wall_clock64(); }   // (trace: the device's 100 MHz clock)

// Step launches of one chunk: kChunk per graph replay; with no_graph the option debug_chunk (a finer control-block trace).
// Every chunk starts its launches at j = 0 and the kernels rotate control and counter blocks by j % 6, so a chunk is a whole
// number of rotations: debug_chunk is rounded up to a multiple of 6, and a value below 1 (or a NaN) is the default.
int steps_per_chunk(const mnav_ctx* ctx)
{
  const double c = ctx->opt.debug_chunk;
  if (ctx->use_graph || !(c >= 1.0)) return kChunk;
  const double up = 6.0 * std::ceil(std::min(c, 6.0e6) / 6.0);
  return (int)up;
}

template <uint32_t PLANNER>
int run_chunk(mnav_ctx* ctx, uint32_t n, uint32_t G, bool wide)
{
  if (!ctx->use_graph) return launch_steps<PLANNER>(ctx, n, G, steps_per_chunk(ctx), wide);
  const uint64_t key = ((uint64_t)PLANNER << 60) | ((uint64_t)(wide ? ctx->wide_groups : 0u) << 57) | ((uint64_t)n << 32) | G;
  auto it = ctx->graphs.find(key);
  if (it == ctx->graphs.end()) {
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    const int rc = launch_steps<PLANNER>(ctx, n, G, kChunk, wide);
    hipError_t e = hipStreamEndCapture(ctx->stream, &g);
    if (rc != 0 || e != hipSuccess) { ctx->err = "graph capture failed"; return -1; }
    GraphExec ge;
    HIPCHK(hipGraphInstantiate(ge.out(), g, nullptr, nullptr, 0));
    (void)hipGraphDestroy(g);
    it = ctx->graphs.emplace(key, std::move(ge)).first;
  }
  HIPCHK(hipGraphLaunch(it->second, ctx->stream));
  return 0;
}

int materialize(mnav_ctx* ctx, bool cvp, double cost_limit)
{
  const uint32_t V = ctx->V;
  const uint32_t gb = (V + kBlock - 1) / kBlock;
  if (!cvp) {
    if (ctx->nbr_valid && ctx->nbr_limit == cost_limit) return 0;
    if (!ctx->d_nbr) HIPCHK(ctx->d_nbr.alloc(sizeof(Nbr) * (size_t)(ctx->E ? 2 * (size_t)ctx->E : 1)));
    hipLaunchKernelGGL(k_build_nbr, dim3(gb ? gb : 1), dim3(kBlock), 0, ctx->stream, V, ctx->d_row_ptr, ctx->d_nbr_u,
                       ctx->d_nbr_e, ctx->d_w, ctx->d_cost, ctx->d_invalid, cost_limit, ctx->d_nbr);
    HIPCHK(hipGetLastError());
    ctx->nbr_limit = cost_limit; ctx->nbr_valid = true; ctx->tw_valid = false; ctx->tb.w_valid = false;
  } else {
    if (ctx->crn_valid && ctx->crn_limit == cost_limit) return 0;
    if (!ctx->d_crn) HIPCHK(ctx->d_crn.alloc(sizeof(Corner) * (size_t)(ctx->F ? 3 * (size_t)ctx->F : 1)));
    if (!ctx->d_blocked) HIPCHK(ctx->d_blocked.alloc(V ? V : 1));
    hipLaunchKernelGGL(k_build_crn, dim3(gb ? gb : 1), dim3(kBlock), 0, ctx->stream, V, ctx->d_crn_ptr, ctx->d_crn_idx,
                       ctx->d_w, ctx->d_cost, ctx->d_invalid, cost_limit, ctx->d_crn, ctx->d_blocked);
    HIPCHK(hipGetLastError());
    ctx->crn_limit = cost_limit; ctx->crn_valid = true;
  }
  return 0;
}

// k_cvp_verify until a sweep finds every vertex at its fixed point: sweeps that find stale deep-cascade members store
// the re-evaluated state (verify_entry) and are followed by another one; the last allowed sweep only checks.
int verify_sweeps(mnav_ctx* ctx, uint32_t n)
{
  if (!ctx->d_verify_any) HIPCHK(ctx->d_verify_any.alloc(4));
  uint32_t gv = (ctx->V / kGroupsPerWave + 3) / 4;                  // ~4 vertices per 8-lane group
  if (gv < 1) gv = 1;
  if (gv > 8192) gv = 8192;
  ctx->verify_sweeps_used = 0;
  for (int sweep = 0; sweep <= kVerifySweeps; ++sweep) {
    uint32_t any = 0;
    HIPCHK(hipMemsetAsync(ctx->d_verify_any, 0, 4, ctx->stream));
    hipLaunchKernelGGL(k_flags_reset, dim3(n), dim3(64), 0, ctx->stream, ctx->d_plans);
    hipLaunchKernelGGL(k_cvp_verify, dim3(gv, n), dim3(kWave), 0, ctx->stream, ctx->d_plans, sweep < kVerifySweeps ? 1 : 0, ctx->d_verify_any);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&any, ctx->d_verify_any, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (any && n == 1 && opt_on(ctx->opt.trace)) {
      Cnt f{};
      (void)hipMemcpy(&f, ctx->slots[0].cnt + 3, sizeof(Cnt), hipMemcpyDeviceToHost);
      fprintf(stderr, "[mnav] verification sweep %d: %u vertices not at their fixed point\n", sweep, f.changed);
    }
    if (!any) break;
    ++ctx->verify_sweeps_used;
  }
  if (ctx->verify_sweeps_used > (uint32_t)kVerifySweeps && n == 1) {
    // the concurrent sweeps keep a tie cluster flipping: list what is off (fix == 2), repair it one vertex at a time, check again
    uint32_t any = 0;
    HIPCHK(hipMemsetAsync(ctx->d_verify_any, 0, 4, ctx->stream));
    hipLaunchKernelGGL(k_flags_reset, dim3(n), dim3(64), 0, ctx->stream, ctx->d_plans);
    hipLaunchKernelGGL(k_cvp_verify, dim3(gv, n), dim3(kWave), 0, ctx->stream, ctx->d_plans, 2, ctx->d_verify_any);
    hipLaunchKernelGGL(k_verify_serial, dim3(n), dim3(kWave), 0, ctx->stream, ctx->d_plans, 200000u);
    HIPCHK(hipMemsetAsync(ctx->d_verify_any, 0, 4, ctx->stream));
    hipLaunchKernelGGL(k_flags_reset, dim3(n), dim3(64), 0, ctx->stream, ctx->d_plans);
    hipLaunchKernelGGL(k_cvp_verify, dim3(gv, n), dim3(kWave), 0, ctx->stream, ctx->d_plans, 0, ctx->d_verify_any);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&any, ctx->d_verify_any, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (opt_on(ctx->opt.trace)) fprintf(stderr, "[mnav] verification: serial repair, %s\n", any ? "still off" : "clean");
  }
  if (opt_on(ctx->opt.trace)) fprintf(stderr, "[mnav] verification: %u fixing sweep(s)\n", ctx->verify_sweeps_used);
  return 0;
}

#include "mnav_engines_host.h"

#include "mnav_tb_host.h"

float ev_ms(hipEvent_t a, hipEvent_t b)
{
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return 0.f;
  return ms;
}

void finish_stats(mnav_ctx* ctx, uint32_t n, bool cvp)
{
  mnav_stats& st = ctx->stats;
  st.n_plans = n;
  st.steps = 0; st.bands = 0; st.armed = 0; st.goal_dist = INFINITY; st.settled = 0; st.evals = 0; st.band_shrinks = 0; st.band_cuts = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const PlanResult& r = ctx->h_res[i];
    if (r.steps > st.steps) st.steps = r.steps;
    if (r.bands > st.bands) st.bands = r.bands;
    st.band_shrinks += r.shrinks & 0xFFFFu; st.band_cuts += r.shrinks >> 16;
    st.armed += r.armed;
    if (i == 0) st.goal_dist = r.goal_dist;
    st.settled += r.settled;
    st.evals += r.evals;
  }
  st.ms_init = ev_ms(ctx->ev[1], ctx->ev[2]);
  st.ms_propagation = ev_ms(ctx->ev[2], ctx->ev[3]);
  st.ms_path = ev_ms(ctx->ev[3], ctx->ev[4]);
  st.ms_vector_map = ev_ms(ctx->ev[4], ctx->ev[5]);
  st.ms_download = ev_ms(ctx->ev[5], ctx->ev[6]);
  st.ms_total = ev_ms(ctx->ev[0], ctx->ev[6]);
  st.ms_step_kernels = (float)ctx->ms_chunks;
  // early-exit variant = settled vertices and their incident edges / faces
  const double V = ctx->V ? ctx->V : 1;
  const double frac = (double)st.settled / V;   // summed over plans
  if (!cvp) ctx->algo_bytes = (uint64_t)(24.0 * st.settled + 24.0 * frac * ctx->E);
  else ctx->algo_bytes = (uint64_t)(32.0 * st.settled + 68.0 * frac * ctx->F);
}

int check_ready(mnav_ctx* ctx)
{
  if (!ctx) return -1;
  if (!ctx->have_mesh) { ctx->err = "mnav_upload_mesh has not been called"; return -1; }
  if (!ctx->have_costs) { ctx->err = "mnav_upload_costs has not been called"; return -1; }
  return 0;
}

// -- change log of the replan -----------------------------------------------------------------------
// Nothing is logged before the first Dijkstra call, and nothing once "everything changed" is set: both are decided here.
uint32_t replan_log_room(mnav_ctx* ctx, uint32_t n)
{
  mnav_ctx::Replan& R = ctx->rp;
  if (!ctx->res.has_recorded_call() || R.all || n == 0) return 0;
  const uint32_t cap = std::min(opt_u32(ctx->opt.replan_log_cap, ctx->V), ctx->V);
  if (n > cap || R.len > cap - n) { R.all = true; return 0; }        // overflow: the next replan plans afresh
  if (!R.log && R.log.alloc(sizeof(uint32_t) * (size_t)(ctx->V ? ctx->V : 1)) != hipSuccess) { R.all = true; return 0; }
  return n;
}
// n vertex ids that are already on the device (enqueued on the context's stream, before the writer's synchronisation)
void replan_log_vertices(mnav_ctx* ctx, const uint32_t* d_ids, uint32_t n)
{
  mnav_ctx::Replan& R = ctx->rp;
  if (!replan_log_room(ctx, n)) return;
  if (hipMemcpyAsync(R.log + R.len, d_ids, sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) { R.all = true; return; }
  R.len += n;
}
// both endpoints of n edges
void replan_log_edges(mnav_ctx* ctx, const uint32_t* d_edge_ids, uint32_t n)
{
  mnav_ctx::Replan& R = ctx->rp;
  if (n > 0x7FFFFFFFu || !replan_log_room(ctx, 2u * n)) { if (n > 0x7FFFFFFFu) R.all = true; return; }
  hipLaunchKernelGGL(k_replan_log_edges, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, n, d_edge_ids, ctx->d_edge_vtx, R.log + R.len);
  if (hipGetLastError() != hipSuccess) { R.all = true; return; }
  R.len += 2u * n;
}

// -- the record of the resident outputs (mnav_resident.h): the context's half of its transitions ------------------------
// Outputs begin (ctx->res.outputs_begin / repair_begin / shard_took_slot0): whatever still names the previous call's device
// memory is void -- the lazy settled-vertex count and the arguments of a tile-batch call, the predecessors of a sharded
// plan -- and so is what mnav_last_engine said about a replan.
void resident_outputs_begin(mnav_ctx* ctx)
{
  ctx->shard.finalized = false; ctx->tb.count_pending = false; ctx->tb_args_valid = false;
  ctx->rp.each_engines = 0; ctx->rp.warm.live = false;
  ctx->mesh_since_outputs = false;
}
// A Dijkstra call or a repair committed (ctx->res.commit_dijkstra / repair_commit): the change log starts over.
void resident_outputs_commit(mnav_ctx* ctx) { ctx->rp.len = 0; ctx->rp.all = false; }

// A stale cancel flag does not cancel the call that starts (dijkstra :238, cvp :679).
void cancel_reset(mnav_ctx* ctx)
{
  ctx->cancel.store(0);
  if (ctx->d_cancel) { (void)hipStreamSynchronize(ctx->cancel_stream); (void)hipMemsetAsync(ctx->d_cancel, 0, 4, ctx->stream); }
}

// the face tables that the device back-tracking and the containing-face search walk: uploaded by whichever comes first
int upload_walk_mesh(mnav_ctx* ctx)
{
  if (ctx->walk_mesh_valid) return 0;
  HIPCHK(ctx->d_faces.upload(ctx->stream, ctx->h_faces.data(), ctx->h_faces.size()));
  HIPCHK(ctx->d_vf_ptr.upload(ctx->stream, ctx->h_vf_ptr.data(), ctx->h_vf_ptr.size()));
  HIPCHK(ctx->d_vf.upload(ctx->stream, ctx->h_vf.data(), ctx->h_vf.size()));
  ctx->walk_mesh_valid = true;
  return 0;
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

mnav_ctx* mnav_create(int device)
{
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return nullptr;
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  mnav_ctx* ctx = new mnav_ctx();
  ctx->device = device;
  if (hipStreamCreateWithFlags(ctx->stream.out(), hipStreamNonBlocking) != hipSuccess) { delete ctx; return nullptr; }
  for (auto& e : ctx->ev)
    if (hipEventCreate(e.out()) != hipSuccess) { delete ctx; return nullptr; }
  for (auto& e : ctx->evc)
    if (hipEventCreate(e.out()) != hipSuccess) { delete ctx; return nullptr; }
  if (ctx->d_seed_pos.alloc(3 * sizeof(float)) != hipSuccess) { delete ctx; return nullptr; }
  if (ctx->d_cancel.alloc(64) != hipSuccess || hipMemset(ctx->d_cancel, 0, 64) != hipSuccess || ctx->h_one.alloc(64) != hipSuccess ||
      hipStreamCreateWithFlags(ctx->cancel_stream.out(), hipStreamNonBlocking) != hipSuccess) { delete ctx; return nullptr; }
  *ctx->h_one = 1u;
  if (ctx->h_actl.alloc(sizeof(AsyncCtl)) != hipSuccess) { delete ctx; return nullptr; }
  ctx->opt.from_environment();                                        // the ONLY look at the environment (mnav_options.h)
  apply_options(ctx);
  return ctx;
}

void mnav_destroy(mnav_ctx* ctx)
{
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->cancel_stream) (void)hipStreamSynchronize(ctx->cancel_stream);
  for (auto& st : ctx->stream_g) if (st) (void)hipStreamSynchronize(st);
  if (ctx->tb.fill_stream) (void)hipStreamSynchronize(ctx->tb.fill_stream);
  delete ctx;                                                         // the owners free the rest
}

const char* mnav_last_error(const mnav_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int mnav_set_face_circulation(mnav_ctx* ctx, uint32_t V, uint32_t F, const uint32_t* vf_ptr, const uint32_t* vf)
{
  if (!ctx) return -1;
  ctx->err.clear();
  ctx->circ = FaceCirculation();
  if (!vf_ptr || !vf) return 0;                                  // back to the built-in half-edge replay
  ctx->circ.ptr.assign(vf_ptr, vf_ptr + (size_t)V + 1);
  ctx->circ.faces.assign(vf, vf + 3 * (size_t)F);
  ctx->circ.ok = true;
  return 0;
}

int mnav_upload_mesh(mnav_ctx* ctx, uint32_t V, uint32_t F, uint32_t E, const float* xyz, const uint32_t* face_vtx,
                     const uint32_t* edge_vtx, const float* vertex_normals)
{
  if (!ctx) return -1;
  ctx->err.clear();
  if ((V && !xyz) || (F && !face_vtx) || (E && !edge_vtx)) { ctx->err = "null mesh array"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  HostTopology t;
  try {
    if (!ctx->circ.ptr.empty()) {
      if (ctx->circ.ptr.size() != (size_t)V + 1 || ctx->circ.faces.size() != 3 * (size_t)F || ctx->circ.ptr[V] != 3 * (size_t)F)
        throw std::invalid_argument("face circulation does not fit this mesh");
      t = build_topology(V, F, E, face_vtx, edge_vtx, &ctx->circ);
    } else {
      t = build_topology(V, F, E, face_vtx, edge_vtx);
    }
  }
  catch (const std::exception& ex) { ctx->err = ex.what(); return -2; }
  (void)hipStreamSynchronize(ctx->stream);
  // V-, E- and F-sized state of the old mesh
  ctx->slots.clear(); ctx->mesh_since_outputs = true;
  ctx->rp.log.reset(); ctx->rp.len = 0; ctx->rp.all = false; ctx->res.mesh_replaced();   // (the log is V-sized; the recorded seeds are the old mesh's)
  ctx->layers.clear();
  ctx->d_crn_infl.reset(); ctx->d_infl_mask.reset(); ctx->d_zero_u8.reset(); ctx->d_infl_keyd.reset(); ctx->crn_infl_valid = false;
  ctx->obs = {};                                                     // rebuilt lazily
  ctx->nbhd = {};                                                    // V-sized spill lists
  ctx->clr = {};                                                     // cached clearance: recast lazily
  ctx->chg = {};                                                     // V-sized change list
  ctx->traffic = {};                                                 // V counts: zero again
  ctx->timed = {};                                                   // V x B cells and holders, V peaks: gone
  ctx->schedule = {};                                                // ... and the schedule's tentative arrays with them
  ctx->map = {};                                                     // the layer graph: its slots are gone
  ctx->loc = {};                                                     // vertex index: rebuilt lazily
  ctx->rp = {};                                                      // change log and replan state: the fields are gone with the slots
  ctx->d_edge_dist.reset();
  drop_graphs(ctx);
  ctx->d_paths.reset(); ctx->paths_words = 0;
  ctx->d_nbr.reset(); ctx->d_crn.reset(); ctx->d_blocked.reset();
  ctx->d_cost.reset(); ctx->d_w.reset(); ctx->d_invalid.reset();
  ctx->nbr_valid = ctx->crn_valid = false; ctx->have_costs = false;
  ctx->V = V; ctx->F = F; ctx->E = E;
  {
    // a planar wavefront needs a few steps per hop of the mesh diameter ~ sqrt(V); generous cap
    const double cap = 400.0 * std::sqrt((double)V) + 20000.0;
    ctx->max_steps = cap > 2.0e9 ? 2000000000u : (uint32_t)cap;
    ctx->max_steps_auto = ctx->max_steps;
    apply_options(ctx);
  }
  ctx->h_xyz.assign(xyz, xyz + 3 * (size_t)V);
  ctx->h_faces.assign(face_vtx, face_vtx + 3 * (size_t)F);
  ctx->h_row_ptr = t.row_ptr; ctx->h_nbr_u = t.nbr_u;
  ctx->h_vf_ptr = std::move(t.vf_ptr); ctx->h_vf = std::move(t.vf); ctx->walk_mesh_valid = false;
  tb_free(ctx);
  HIPCHK(ctx->d_row_ptr.upload(ctx->stream, t.row_ptr.data(), t.row_ptr.size()));
  HIPCHK(ctx->d_nbr_u.upload(ctx->stream, t.nbr_u.data(), t.nbr_u.size()));
  HIPCHK(ctx->d_nbr_e.upload(ctx->stream, t.nbr_e.data(), t.nbr_e.size()));
  HIPCHK(ctx->d_crn_ptr.upload(ctx->stream, t.crn_ptr.data(), t.crn_ptr.size()));
  HIPCHK(ctx->d_edge_vtx.upload(ctx->stream, edge_vtx, 2 * (size_t)E));
  std::vector<CornerIdx> ci(t.crn_v1.size());
  for (size_t i = 0; i < ci.size(); ++i) ci[i] = CornerIdx{ t.crn_v1[i], t.crn_v2[i], t.crn_ea[i], t.crn_eb[i], t.crn_ec[i], t.crn_face[i] };
  HIPCHK(ctx->d_crn_walk.upload(ctx->stream, t.crn_walk.data(), t.crn_walk.size()));
  HIPCHK(ctx->d_crn_idx.upload(ctx->stream, ci.data(), ci.size()));
  HIPCHK(ctx->d_xyz.upload(ctx->stream, xyz, 3 * (size_t)V));
  ctx->have_normals = vertex_normals != nullptr;
  ctx->d_fnrm.reset(); ctx->have_face_normals = false;               // the old mesh's face normals
  HIPCHK(ctx->d_nrm.upload(ctx->stream, vertex_normals, vertex_normals ? 3 * (size_t)V : 0));
  // LDS tiles of the SSSP engine
  {
    ctx->tile_size = opt_u32(ctx->opt.tile_size, 512u);
    if (ctx->tile_size < 64) ctx->tile_size = 64;
    if (ctx->tile_size > (uint32_t)(kTileBlock * kTileVpt)) ctx->tile_size = kTileBlock * kTileVpt;
    HostTiles T;
    for (;;) {
      try { T = build_tiles(t, xyz, ctx->tile_size); }
      catch (const std::exception& ex) { ctx->err = ex.what(); return -2; }
      ctx->tile_lds = tile_lds_bytes(T.max_nv, T.max_nh, T.max_ne);
      ctx->fin_lds = finalize_lds_bytes(T.max_nv, T.max_nh, T.max_ne);
      if (ctx->fin_lds <= 150 * 1024 || ctx->tile_size <= 64) break;
      ctx->tile_size /= 2;                       // irregular mesh: shrink until a tile fits the 160 KiB LDS
    }
    if (ctx->fin_lds > 160 * 1024) { ctx->err = "mesh valence too high for the LDS tile engine"; return -2; }
    if (ctx->fin_lds > 64 * 1024)
      HIPCHK(hipFuncSetAttribute((const void*)k_dij_finalize, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ctx->fin_lds));
    if (ctx->tile_lds > 64 * 1024)
      HIPCHK(hipFuncSetAttribute((const void*)k_tile_round, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ctx->tile_lds));
    if (ctx->tile_lds > 64 * 1024) {
      HIPCHK(hipFuncSetAttribute((const void*)k_plan_async<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ctx->tile_lds));
      HIPCHK(hipFuncSetAttribute((const void*)k_plan_async<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ctx->tile_lds));
      HIPCHK(hipFuncSetAttribute((const void*)k_plan_async<8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ctx->tile_lds));
    }
    if (opt_on(ctx->opt.verbose))
      fprintf(stderr, "[mnav] tiles: size %u, %u tiles, max owned %u, halo %u, edges %u -> LDS %zu B (solve), %zu B (finalize)\n",
              ctx->tile_size, T.ntiles, T.max_nv, T.max_nh, T.max_ne, ctx->tile_lds, ctx->fin_lds);
    ctx->d_t_tw.reset(); ctx->tw_valid = false;
    ctx->t_nnz = (uint32_t)T.col.size();
    HIPCHK(ctx->d_t_vptr.upload(ctx->stream, T.vptr.data(), T.vptr.size()));
    HIPCHK(ctx->d_t_verts.upload(ctx->stream, T.verts.data(), T.verts.size()));
    HIPCHK(ctx->d_t_hptr.upload(ctx->stream, T.hptr.data(), T.hptr.size()));
    HIPCHK(ctx->d_t_halo_verts.upload(ctx->stream, T.halo_verts.data(), T.halo_verts.size()));
    HIPCHK(ctx->d_t_halo_tile.upload(ctx->stream, T.halo_tile.data(), T.halo_tile.size()));
    HIPCHK(ctx->d_t_eptr.upload(ctx->stream, T.eptr.data(), T.eptr.size()));
    HIPCHK(ctx->d_t_rptr.upload(ctx->stream, T.rptr.data(), T.rptr.size()));
    HIPCHK(ctx->d_t_rowptr.upload(ctx->stream, T.rowptr.data(), T.rowptr.size()));
    HIPCHK(ctx->d_t_col.upload(ctx->stream, T.col.data(), T.col.size()));
    HIPCHK(ctx->d_t_src.upload(ctx->stream, T.src.data(), T.src.size()));
    HIPCHK(ctx->d_vert_tile.upload(ctx->stream, T.vert_tile.data(), T.vert_tile.size()));
    HIPCHK(ctx->d_t_tw.upload(ctx->stream, nullptr, T.col.size()));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    // keep the sizes, and the small per-vertex maps the partitioner of mnav_shard_setup needs, on the host
    T.halo_tile.clear(); T.halo_tile.shrink_to_fit(); T.rowptr.clear(); T.rowptr.shrink_to_fit();
    T.col.clear(); T.col.shrink_to_fit(); T.src.clear(); T.src.shrink_to_fit();
    ctx->tiles_meta = std::move(T);
    ctx->shard.ready = false;
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));   // host vectors go out of scope
  ctx->have_mesh = true;
  return 0;
}

static void auto_delta(mnav_ctx* ctx, const float* w, uint32_t E)
{
  double s = 0; uint64_t c = 0;
  for (uint32_t e = 0; e < E; ++e) if (std::isfinite(w[e])) { s += w[e]; ++c; }
  ctx->delta_auto = c ? (float)(3.0 * s / (double)c) : 1.0f;
  if (!(ctx->delta_auto > 0.f)) ctx->delta_auto = 1.0f;
  // tile band ~ the potential difference across one tile (sqrt(tile_size) mean edges)
  ctx->tile_band_auto = (ctx->delta_auto / 3.0f) * std::sqrt((float)ctx->tile_size);
}

int mnav_upload_costs(mnav_ctx* ctx, const float* vertex_costs, const float* edge_weights, const uint8_t* invalid)
{
  if (!ctx) return -1;
  ctx->err.clear();
  if (!ctx->have_mesh) { ctx->err = "mnav_upload_mesh has not been called"; return -1; }
  if ((ctx->V && !vertex_costs) || (ctx->E && !edge_weights)) { ctx->err = "null cost array"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  ctx->rp.all = true;                                                // whole arrays replaced: a replan plans afresh, also after a failure half way
  HIPCHK(ctx->d_cost.upload(ctx->stream, vertex_costs, ctx->V));
  HIPCHK(ctx->d_w.upload(ctx->stream, edge_weights, ctx->E));
  std::vector<uint8_t> zero;
  if (!invalid) { zero.assign(ctx->V ? ctx->V : 1, 0); invalid = zero.data(); }
  HIPCHK(ctx->d_invalid.upload(ctx->stream, invalid, ctx->V));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->h_cost.assign(vertex_costs, vertex_costs + ctx->V);
  ctx->h_invalid.assign(invalid, invalid + ctx->V);
  auto_delta(ctx, edge_weights, ctx->E);
  ctx->nbr_valid = ctx->crn_valid = false;
  ctx->have_costs = true;
  ctx->edge_cost_factor = 0.0;                                       // weights came from the caller: mnav_update_costs only touches vertex costs
  return 0;
}

// device pass shared by mnav_compute_edge_weights / mnav_combine_costs: d_cost and d_edge_dist are resident, d_w is
// (re)computed; host mirrors (cost for the seed cut-offs, mean weight for the band widths) are refreshed
static int edge_weight_pass(mnav_ctx* ctx, double edge_cost_factor, const uint8_t* invalid, float* vertex_costs_out, float* edge_weights_out)
{
  ctx->rp.all = true;                                                // whole arrays replaced: a replan plans afresh
  HIPCHK(ctx->d_w.upload(ctx->stream, nullptr, ctx->E));
  std::vector<uint8_t> zero;
  if (!invalid) { zero.assign(ctx->V ? ctx->V : 1, 0); invalid = zero.data(); }
  HIPCHK(ctx->d_invalid.upload(ctx->stream, invalid, ctx->V));
  const uint32_t gb = (ctx->E + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_edge_weights, dim3(gb ? gb : 1), dim3(kBlock), 0, ctx->stream, ctx->E, ctx->d_edge_vtx, ctx->d_edge_dist,
                     ctx->d_cost, edge_cost_factor, ctx->d_w);
  HIPCHK(hipGetLastError());
  std::vector<float> w(ctx->E ? ctx->E : 1);
  ctx->h_cost.resize(ctx->V);
  HIPCHK(hipMemcpyAsync(w.data(), ctx->d_w, sizeof(float) * ctx->E, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->h_cost.data(), ctx->d_cost, sizeof(float) * ctx->V, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (edge_weights_out) memcpy(edge_weights_out, w.data(), sizeof(float) * ctx->E);
  if (vertex_costs_out) memcpy(vertex_costs_out, ctx->h_cost.data(), sizeof(float) * ctx->V);
  ctx->h_invalid.assign(invalid, invalid + ctx->V);
  auto_delta(ctx, w.data(), ctx->E);
  ctx->nbr_valid = ctx->crn_valid = false;
  ctx->edge_cost_factor = edge_cost_factor;
  ctx->have_costs = true;
  return 0;
}

int mnav_compute_edge_weights(mnav_ctx* ctx, const float* vertex_costs, const float* edge_distances, double edge_cost_factor,
                              const uint8_t* invalid, float* edge_weights_out)
{
  if (!ctx) return -1;
  ctx->err.clear();
  if (!ctx->have_mesh) { ctx->err = "mnav_upload_mesh has not been called"; return -1; }
  if ((ctx->V && !vertex_costs) || (ctx->E && !edge_distances)) { ctx->err = "null cost array"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  ctx->rp.all = true;                                                // whole arrays replaced: a replan plans afresh, also after a failure half way
  HIPCHK(ctx->d_cost.upload(ctx->stream, vertex_costs, ctx->V));
  HIPCHK(ctx->d_edge_dist.upload(ctx->stream, edge_distances, ctx->E));
  ctx->crn_infl_valid = false;
  return edge_weight_pass(ctx, edge_cost_factor, invalid, nullptr, edge_weights_out);
}

int mnav_combine_costs(mnav_ctx* ctx, int mode, uint32_t n_layers, const float* const* layer_costs, const float* weights,
                       const float* edge_distances, double edge_cost_factor, const uint8_t* invalid, float* vertex_costs_out,
                       float* edge_weights_out)
{
  if (!ctx) return -1;
  ctx->err.clear();
  if (!ctx->have_mesh) { ctx->err = "mnav_upload_mesh has not been called"; return -1; }
  if (mode != 0 && mode != 1) { ctx->err = "combination mode must be 0 (max) or 1 (weighted sum)"; return -1; }
  if ((n_layers && !layer_costs) || (mode == 1 && n_layers && !weights) || (ctx->E && !edge_distances && !ctx->d_edge_dist)) { ctx->err = "null input array"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  ctx->rp.all = true;                                                // whole arrays replaced: a replan plans afresh, also after a failure half way
  const uint32_t V = ctx->V;
  DevBuf<float> d_layers, d_wts;
  HIPCHK(d_layers.alloc(sizeof(float) * ((size_t)n_layers * V + 1)));
  HIPCHK(d_wts.alloc(sizeof(float) * (n_layers + 1)));
  int rc = 0;
  for (uint32_t l = 0; l < n_layers && rc == 0; ++l) {
    if (!layer_costs[l]) { ctx->err = "null layer"; rc = -1; break; }
    if (hipMemcpyAsync(d_layers + (size_t)l * V, layer_costs[l], sizeof(float) * V, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { ctx->err = "layer upload failed"; rc = -1; }
  }
  if (rc == 0 && mode == 1 && n_layers &&
      hipMemcpyAsync(d_wts, weights, sizeof(float) * n_layers, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { ctx->err = "weight upload failed"; rc = -1; }
  if (rc == 0 && ctx->d_cost.upload(ctx->stream, nullptr, V) != hipSuccess) { ctx->err = "cost buffer allocation failed"; rc = -1; }
  if (rc == 0 && edge_distances) {                                   // NULL: keep the resident ones
    ctx->crn_infl_valid = false;
    if (ctx->d_edge_dist.upload(ctx->stream, edge_distances, ctx->E) != hipSuccess) { ctx->err = "edge distance upload failed"; rc = -1; }
  }
  if (rc == 0) {
    const uint32_t gb = (V + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_combine, dim3(gb ? gb : 1), dim3(kBlock), 0, ctx->stream, V, mode, n_layers, d_layers, d_wts, ctx->d_cost);
    if (hipGetLastError() != hipSuccess) { ctx->err = "cost combination failed"; rc = -1; }
  }
  // the combined costs never leave the device: the edge-weight pass reads them where they are
  if (rc == 0) rc = edge_weight_pass(ctx, edge_cost_factor, invalid, vertex_costs_out, edge_weights_out);
  (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

int mnav_update_costs(mnav_ctx* ctx, uint32_t n, const uint32_t* vertex_ids, const float* values)
{
  if (!ctx) return -1;
  ctx->err.clear();
  if (!ctx->have_costs) { ctx->err = "no costs resident yet (mnav_upload_costs / mnav_compute_edge_weights / mnav_combine_costs first)"; return -1; }
  if (n == 0) return 0;
  if (!vertex_ids || !values) { ctx->err = "null input array"; return -1; }
  for (uint32_t i = 0; i < n; ++i) if (vertex_ids[i] >= ctx->V) { ctx->err = "vertex id out of range"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  DevBuf<uint32_t> d_ids; DevBuf<float> d_vals;
  HIPCHK(d_ids.alloc(sizeof(uint32_t) * n));
  HIPCHK(d_vals.alloc(sizeof(float) * n));
  int rc = 0;
  if (hipMemcpyAsync(d_ids, vertex_ids, sizeof(uint32_t) * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      hipMemcpyAsync(d_vals, values, sizeof(float) * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { ctx->err = "upload failed"; rc = -1; }
  if (rc == 0) {
    hipLaunchKernelGGL(k_scatter_costs, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, n, d_ids, d_vals, ctx->d_cost);
    // "Edge costs are only affected by vertex costs if layer_factor is not 0" (:568-572)
    if (ctx->edge_cost_factor != 0.0) {
      if (!ctx->d_edge_dist) { ctx->err = "edge distances are not resident (weights were uploaded, not computed here)"; rc = -1; }
      else hipLaunchKernelGGL(k_update_edge_weights, dim3((8 * n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, n, d_ids, ctx->d_row_ptr,
                              ctx->d_nbr_u, ctx->d_nbr_e, ctx->d_edge_dist, ctx->d_cost, ctx->edge_cost_factor, ctx->d_w);
    }
    if (rc == 0 && hipGetLastError() != hipSuccess) { ctx->err = "cost update failed"; rc = -1; }
    if (rc == 0) replan_log_vertices(ctx, d_ids, n);
  }
  if (rc) ctx->rp.all = true;                                        // (how far a failed update got is unknown)
  (void)hipStreamSynchronize(ctx->stream);
  if (rc) return rc;
  for (uint32_t i = 0; i < n; ++i) ctx->h_cost[vertex_ids[i]] = values[i];
  ctx->nbr_valid = ctx->crn_valid = false;                          // the cost-limit folded copies are rebuilt on the next plan
  return 0;
}

int mnav_update_edge_weights(mnav_ctx* ctx, uint32_t n, const uint32_t* edge_ids, const float* values)
{
  if (!ctx) return -1;
  ctx->err.clear();
  if (!ctx->have_costs) { ctx->err = "no costs resident yet (mnav_upload_costs / mnav_compute_edge_weights / mnav_combine_costs first)"; return -1; }
  if (n == 0) return 0;
  if (!edge_ids || !values) { ctx->err = "null input array"; return -1; }
  for (uint32_t i = 0; i < n; ++i) if (edge_ids[i] >= ctx->E) { ctx->err = "edge id out of range"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  DevBuf<uint32_t> d_ids; DevBuf<float> d_vals;
  HIPCHK(d_ids.alloc(sizeof(uint32_t) * n));
  HIPCHK(d_vals.alloc(sizeof(float) * n));
  int rc = 0;
  if (hipMemcpyAsync(d_ids, edge_ids, sizeof(uint32_t) * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      hipMemcpyAsync(d_vals, values, sizeof(float) * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { ctx->err = "upload failed"; rc = -1; }
  if (rc == 0) {
    hipLaunchKernelGGL(k_scatter_costs, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, n, d_ids, d_vals, ctx->d_w);   // (a scatter of floats by index)
    if (hipGetLastError() != hipSuccess) { ctx->err = "edge weight update failed"; rc = -1; }
    if (rc == 0) replan_log_edges(ctx, d_ids, n);
  }
  if (rc) ctx->rp.all = true;                                        // (how far a failed update got is unknown)
  (void)hipStreamSynchronize(ctx->stream);
  if (rc) return rc;
  ctx->nbr_valid = ctx->crn_valid = false;                          // the cost-limit folded copies (and the tiles' weights behind them) are rebuilt on the next plan
  return 0;
}

int mnav_download_costs(mnav_ctx* ctx, float* vertex_costs_out, float* edge_weights_out)
{
  if (!ctx || !ctx->have_costs) { if (ctx) ctx->err = "no costs resident"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) return -1;
  if (vertex_costs_out) HIPCHK(hipMemcpyAsync(vertex_costs_out, ctx->d_cost, sizeof(float) * ctx->V, hipMemcpyDeviceToHost, ctx->stream));
  if (edge_weights_out) HIPCHK(hipMemcpyAsync(edge_weights_out, ctx->d_w, sizeof(float) * ctx->E, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

// -- layers on the device ------------------------------------------------------------------------
static int layer_slot(mnav_ctx* ctx, uint32_t layer, bool want_dist)
{
  if (!ctx->have_mesh) { ctx->err = "mnav_upload_mesh has not been called"; return -1; }
  if (layer >= 64) { ctx->err = "layer index out of range (64 layers)"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  if (ctx->layers.size() <= layer) ctx->layers.resize(layer + 1);
  mnav_ctx::Layer& L = ctx->layers[layer];
  const size_t V = ctx->V ? ctx->V : 1;
  if (!L.cost) HIPCHK(L.cost.alloc(4 * V));
  if (!L.lethal) HIPCHK(L.lethal.alloc(V));
  if (want_dist && !L.dist) HIPCHK(L.dist.alloc(4 * V));
  return 0;
}

// Every writer of a slot but the inflation wave ends here: the slot holds a plain layer, and no wave distances / vector
// field of an earlier inflation layer survive in it.
static void layer_commit_plain(mnav_ctx::Layer& L)
{
  L.have_vec = false;
  L.dist.reset();
  L.ready = true;
}

// the scratch of the change-list pass: V ids, 3 words per block, the counters (once per mesh)
static int change_scratch(mnav_ctx* ctx)
{
  using namespace mnav_chg;
  Scratch& S = ctx->chg;
  const size_t V = ctx->V ? ctx->V : 1, nblk = blocks(ctx->V) ? blocks(ctx->V) : 1;
  if (!S.cnt) HIPCHK(alloc_group(S.ids, sizeof(uint32_t) * V, S.blk, sizeof(uint32_t) * 3 * nblk, S.cnt, sizeof(uint32_t) * kCounters));
  return 0;
}

extern "C++" {
// The pass that ends the obstacle, clearance and border layers (mnav_changelist.h): new costs and flags from `rule`, diffed
// against the slot, written into it, `done` recorded; then the counters of the call (those of its ray cast included)
// into `c`, the ascending change list into `changed_out` and the two totals into `n_changed` / `n_lethal` (each may be null).
template <class Rule>
static int layer_change_list(mnav_ctx* ctx, mnav_ctx::Layer& L, const Rule& rule, hipEvent_t done, uint32_t (&c)[mnav_chg::kCounters],
                             uint32_t* changed_out, uint32_t* n_changed, uint32_t* n_lethal)
{
  using namespace mnav_chg;
  if (change_scratch(ctx)) return -1;
  Scratch& S = ctx->chg;
  const uint32_t V = ctx->V, nblk = blocks(V), fresh = L.ready ? 0u : 1u;
  if (nblk) {
    hipLaunchKernelGGL(k_chg_count<Rule>, dim3(nblk), dim3(kChgBlock), 0, ctx->stream, V, rule, fresh, L.cost, L.lethal, S.blk, nblk);
    hipLaunchKernelGGL(k_chg_scan, dim3(1), dim3(kChgBlock), 0, ctx->stream, nblk, S.blk, S.cnt);
    hipLaunchKernelGGL(k_chg_emit<Rule>, dim3(nblk), dim3(kChgBlock), 0, ctx->stream, V, rule, fresh, L.cost, L.lethal, S.blk, nblk, S.ids);
  } else {
    HIPCHK(hipMemsetAsync(S.cnt + kChanged, 0, sizeof(uint32_t) * 2, ctx->stream));   // no vertex: k_chg_scan sets no totals
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(done, ctx->stream));
  HIPCHK(hipMemcpyAsync(c, S.cnt, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (changed_out && c[kChanged]) {
    HIPCHK(hipMemcpyAsync(changed_out, S.ids, sizeof(uint32_t) * c[kChanged], hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  layer_commit_plain(L);
  if (n_changed) *n_changed = c[kChanged];
  if (n_lethal) *n_lethal = c[kLethal];
  return 0;
}
}  // extern "C++"

static int ensure_edge_distances(mnav_ctx* ctx)
{
  if (ctx->d_edge_dist) return 0;
  HIPCHK(ctx->d_edge_dist.upload(ctx->stream, nullptr, ctx->E));
  const uint32_t gb = (ctx->E + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_edge_dist, dim3(gb ? gb : 1), dim3(kBlock), 0, ctx->stream, ctx->E, ctx->d_edge_vtx, ctx->d_xyz, ctx->d_edge_dist);
  HIPCHK(hipGetLastError());
  ctx->crn_infl_valid = false;
  return 0;
}

int mnav_layer_upload(mnav_ctx* ctx, uint32_t layer, const float* costs, const uint8_t* lethal)
{
  if (!ctx) return -1;
  ctx->err.clear();
  if (layer_slot(ctx, layer, false)) return -1;
  mnav_ctx::Layer& L = ctx->layers[layer];
  if (!costs) { ctx->err = "null cost array"; return -1; }
  HIPCHK(hipMemcpyAsync(L.cost, costs, sizeof(float) * ctx->V, hipMemcpyHostToDevice, ctx->stream));
  if (lethal) HIPCHK(hipMemcpyAsync(L.lethal, lethal, ctx->V, hipMemcpyHostToDevice, ctx->stream));
  else HIPCHK(hipMemsetAsync(L.lethal, 0, ctx->V ? ctx->V : 1, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  layer_commit_plain(L);
  return 0;
}

int mnav_layer_steepness(mnav_ctx* ctx, uint32_t layer, double threshold)
{
  if (!ctx) return -1;
  ctx->err.clear();
  if (layer_slot(ctx, layer, false)) return -1;
  if (!ctx->have_normals) { ctx->err = "vertex normals are not resident (mnav_upload_mesh with vertex_normals)"; return -1; }
  mnav_ctx::Layer& L = ctx->layers[layer];
  const uint32_t gb = (ctx->V + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_steepness, dim3(gb ? gb : 1), dim3(kBlock), 0, ctx->stream, ctx->V, ctx->d_nrm, threshold, L.cost, L.lethal);
  HIPCHK(hipGetLastError());
  layer_commit_plain(L);
  return 0;
}

// InflationLayer::computeLayer (inflation_layer.cpp:96-178 / :577-600): lethals of the input layer -> distances_
// (multi-source wave) -> riskiness.  Runs the wave on the band engine with plan slot 0's work arrays.
// `invalid` is a host array, `d_invalid` the same flags already on the device (the layer graph's); either or neither.
// With `diff` (the layer graph's update path) the slot's costs and flags are not stored plainly: they are diffed against
// the slot while being written (mnav_map::InflRule), and diff->h_cnt holds the counters of that pass on return.
static int layer_inflation_impl(mnav_ctx* ctx, uint32_t layer, uint32_t input_layer, double inflation_radius, double inscribed_radius,
                                double inscribed_value, double lethal_value, double cost_scaling_factor, const uint8_t* invalid,
                                const uint8_t* d_invalid, const mnav_map::Diff* diff)
{
  if (input_layer >= ctx->layers.size() || !ctx->layers[input_layer].ready) { ctx->err = "input layer is not resident"; return -1; }
  if (layer == input_layer) { ctx->err = "a layer cannot inflate itself"; return -1; }
  if (layer_slot(ctx, layer, true)) return -1;
  if (ctx->V > (1u << kKeyIdBits)) { ctx->err = "the ordered wave supports meshes of up to 2^26 vertices"; return -1; }
  if (ensure_edge_distances(ctx)) return -1;
  const uint32_t V = ctx->V;
  const uint32_t gb = (V + kBlock - 1) / kBlock ? (V + kBlock - 1) / kBlock : 1;
  if (!ctx->d_crn_infl) HIPCHK(ctx->d_crn_infl.alloc(sizeof(Corner) * (size_t)(ctx->F ? 3 * (size_t)ctx->F : 1)));
  if (!ctx->crn_infl_valid) {
    hipLaunchKernelGGL(k_build_crn_infl, dim3(gb), dim3(kBlock), 0, ctx->stream, V, ctx->d_crn_ptr, ctx->d_crn_idx, ctx->d_edge_dist, ctx->d_crn_infl);
    HIPCHK(hipGetLastError());
    ctx->crn_infl_valid = true;
  }
  const size_t Vn = V ? V : 1;
  if (!ctx->d_infl_mask) HIPCHK(ctx->d_infl_mask.alloc(Vn));
  if (!ctx->d_zero_u8) { HIPCHK(ctx->d_zero_u8.alloc(Vn)); HIPCHK(hipMemsetAsync(ctx->d_zero_u8, 0, Vn, ctx->stream)); }
  if (!ctx->d_infl_keyd) HIPCHK(ctx->d_infl_keyd.alloc(4 * Vn));
  DevBuf<uint8_t> d_inv;
  if (invalid) { HIPCHK(d_inv.alloc(Vn)); HIPCHK(hipMemcpyAsync(d_inv, invalid, V, hipMemcpyHostToDevice, ctx->stream)); d_invalid = d_inv; }
  mnav_ctx::Layer& L = ctx->layers[layer];
  mnav_ctx::Layer& In = ctx->layers[input_layer];
  L.inflation_radius = inflation_radius; L.inscribed_radius = inscribed_radius; L.inscribed_value = inscribed_value; L.lethal_value = lethal_value;
  hipLaunchKernelGGL(k_infl_mask, dim3(gb), dim3(kBlock), 0, ctx->stream, V, In.lethal, d_invalid, ctx->d_infl_mask);
  if (!diff) HIPCHK(hipMemcpyAsync(L.lethal, In.lethal, V, hipMemcpyDeviceToDevice, ctx->stream));    // lethal_vertices_ = input->lethals() :170,:584
  if (ensure_slots(ctx, 1, true, true, false)) return -1;
  Slot& s = ctx->slots[0];
  ctx->res.wave_took_slot0();                                       // the wave works in plan slot 0: the last plan's resident outputs are gone
  ctx->shard.finalized = false;
  Plan P;
  memset(&P, 0, sizeof(P));
  P.planner = kPlannerCvp; P.V = V;
  P.row_ptr = ctx->d_row_ptr.get(); P.nbr = nullptr; P.crn_ptr = ctx->d_crn_ptr.get(); P.crn = ctx->d_crn_infl.get(); P.blocked = ctx->d_zero_u8.get();
  P.dist = L.dist.get(); P.tkey = s.tkey.get(); P.pred = s.pred.get(); P.dirn = s.dirn.get(); P.cutf = s.cutf.get(); P.stamp = s.stamp.get(); P.dirty = s.dirty.get();
  P.list[0] = s.list0.get(); P.list[1] = s.list1.get(); P.wlist[0] = s.wlist0.get(); P.wlist[1] = s.wlist1.get(); P.wstamp = s.wstamp.get(); P.cap = V; P.ctl = s.ctl; P.cnt = s.cnt.get();
  const float maxd = (float)inflation_radius;                                               // :438 (const float&)
  P.delta = maxd > 0.f ? maxd : 1.0f;                                                       // one band per radius: the wave dies out within ~2
  P.offset = 0.0; P.max_steps = ctx->max_steps; P.walk_max = ctx->walk_max; P.descend_max = ctx->descend_max;
  for (int k = 0; k < 3; ++k) { P.seed[k] = kNone; P.target[k] = kNone; P.seed_d[k] = 0.f; P.seed_expands[k] = 1; P.target_expands[k] = 0; }
  P.seed_face = kNone;
  P.seed_mask = ctx->d_infl_mask.get(); P.keyd = ctx->d_infl_keyd.get(); P.infl_max = maxd;
  HIPCHK(hipMemcpyAsync(ctx->d_plans, &P, sizeof(Plan), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  uint32_t gi = (V + kBlock * 4 - 1) / (kBlock * 4);
  if (gi < 1) gi = 1;
  if (gi > 4096) gi = 4096;
  hipLaunchKernelGGL(k_init<kPlannerCvp>, dim3(gi, 1), dim3(kBlock), 0, ctx->stream, ctx->d_plans);
  hipLaunchKernelGGL(k_infl_ctl, dim3(1), dim3(64), 0, ctx->stream, ctx->d_plans);
  hipLaunchKernelGGL(k_infl_seed, dim3(gi), dim3(kBlock), 0, ctx->stream, ctx->d_plans);
  HIPCHK(hipGetLastError());
  // the wave front of an inflation is as long as the lethal contours, not O(sqrt V): more waves than a plan gets
  uint32_t G = blocks_per_plan(ctx) * 12u;
  if (G > 8192u) G = 8192u;
  const auto t_start = std::chrono::steady_clock::now();
  Ctl last{};
  ctx->infl_exact_bands = 0;
  for (;;) {
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() > ctx->max_wall_s) {
      ctx->err = "inflation wave exceeded the wall-clock guard"; return -1;
    }
    const auto t_c0 = std::chrono::steady_clock::now();
    const bool tr = opt_on(ctx->opt.trace);
    unsigned long long* const stamps = reinterpret_cast<unsigned long long*>(ctx->h_res.get());   // (trace: two device clock stamps in the pinned result record, unused during a wave)
    if (tr) { HIPCHK(hipEventRecord(ctx->ev[4], ctx->stream)); hipLaunchKernelGGL(k_stamp_to_host, dim3(1), dim3(1), 0, ctx->stream, stamps); }   // (trace: the chunk's time on the DEVICE, apart from the host's wait for it)
    if (run_chunk<kPlannerCvp>(ctx, 1, G, false)) return -1;
    if (tr) HIPCHK(hipEventRecord(ctx->ev[5], ctx->stream));
    const auto t_c1 = std::chrono::steady_clock::now();
    if (tr) hipLaunchKernelGGL(k_stamp_to_host, dim3(1), dim3(1), 0, ctx->stream, stamps + 1);
    HIPCHK(hipMemcpyAsync(ctx->h_ctl, ctx->d_ctl_pool, 2 * sizeof(Ctl), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const auto t_c2 = std::chrono::steady_clock::now();
    float dev_ms = 0.f;
    if (tr) (void)hipEventElapsedTime(&dev_ms, ctx->ev[4], ctx->ev[5]);
    last = ctx->h_ctl[0].it > ctx->h_ctl[1].it ? ctx->h_ctl[0] : ctx->h_ctl[1];
    if (opt_on(ctx->opt.trace))
      fprintf(stderr, "[mnav] inflation it %d n %u thr %.6f fixed %.6f width %.4g bands %u band_steps %u shrinks %u cuts %u repair %u evals %u wread %u wbase %u done %u (verify sweeps of the previous wave %u) host ms: since start %.3f, this chunk's launch %.3f, its wait %.3f, the chunk on the device %.3f, by the device's own clock %.3f\n", last.it,
              last.n, last.thr, last.thr_fixed, last.width, last.bands, last.band_steps, last.shrinks, last.cuts, last.repair, last.evals, last.wread, last.wbase, last.done, ctx->verify_sweeps_used,
              1e3 * std::chrono::duration<double>(t_c0 - t_start).count(), 1e3 * std::chrono::duration<double>(t_c1 - t_c0).count(), 1e3 * std::chrono::duration<double>(t_c2 - t_c1).count(), dev_ms, tr ? (double)(stamps[1] - stamps[0]) * 1e-5 : 0.0);
    if (last.done) break;
    if (last.exact_wanted) {
      // a band that neither the concurrent steps nor a serial band from a clean state settle (tied pop times around isolated
      // lethal vertices: 0.5 % of random such maps): its vertices are popped one at a time, the reference's own procedure
      // (mnav_eval.h exact_*; the steps idle meanwhile and resume with a cut step)
      hipLaunchKernelGGL(k_exact_band, dim3(1), dim3(kWave), 0, ctx->stream, ctx->d_plans, (uint32_t*)nullptr);
      HIPCHK(hipGetLastError());
      ++ctx->infl_exact_bands;
    }
  }
  HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
  // verification: every vertex must be a fixed point of the replay rule on the converged state (k_cvp_verify)
  if (verify_sweeps(ctx, 1)) return -1;
  if (diff) {
    using namespace mnav_map;
    const InflRule rule{ L.dist, In.lethal, inflation_radius, inscribed_radius, inscribed_value, lethal_value, cost_scaling_factor };
    const uint32_t nblk = blocks(V) ? blocks(V) : 1, fresh = L.ready ? 0u : 1u;
    hipLaunchKernelGGL(k_node_count<InflRule>, dim3(nblk), dim3(kChgBlock), 0, ctx->stream, V, rule, fresh, L.cost, L.lethal, diff->blk, nblk);
    hipLaunchKernelGGL(k_node_scan, dim3(1), dim3(kChgBlock), 0, ctx->stream, nblk, diff->blk, diff->cnt);
    hipLaunchKernelGGL(k_node_emit<InflRule>, dim3(nblk), dim3(kChgBlock), 0, ctx->stream, V, rule, fresh, L.cost, L.lethal, diff->blk, nblk, diff->ids);
  } else {
    hipLaunchKernelGGL(k_infl_cost, dim3(gb), dim3(kBlock), 0, ctx->stream, V, L.dist, inflation_radius, inscribed_radius, inscribed_value,
                       lethal_value, cost_scaling_factor, L.cost);
  }
  HIPCHK(hipGetLastError());
  // vector_map_ (:277-309): accumulation over the lethal contours, then assignments in pop order (launches until settled)
  L.have_vec = false;
  if (!L.vec) HIPCHK(L.vec.alloc(12 * Vn));
  if (!L.vstate) HIPCHK(L.vstate.alloc(3 * Vn));
  if (!ctx->d_verify_any) HIPCHK(ctx->d_verify_any.alloc(4));
  DevBuf<uint32_t> d_vctl;
  HIPCHK(d_vctl.alloc(16));
  HIPCHK(hipMemsetAsync(d_vctl, 0, 16, ctx->stream));
  uint8_t *st0 = L.vstate, *st1 = L.vstate + Vn, *acc = L.vstate + 2 * Vn;
  hipLaunchKernelGGL(k_infl_accum, dim3(gb), dim3(kBlock), 0, ctx->stream, ctx->d_plans, ctx->d_crn_walk, ctx->d_xyz, L.vec, st0, acc, d_vctl);
  uint32_t vctl[4] = { 0, 0, 0, 0 };
  bool vec_ok = true;
  for (int sweep = 0; sweep < 4096; ++sweep) {
    HIPCHK(hipMemsetAsync(d_vctl, 0, 8, ctx->stream));
    hipLaunchKernelGGL(k_infl_assign, dim3(gb), dim3(kBlock), 0, ctx->stream, ctx->d_plans, L.vec, st0, st1, acc, d_vctl);
    HIPCHK(hipMemcpyAsync(vctl, d_vctl, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::swap(st0, st1);
    if (vctl[2]) { vec_ok = false; break; }                          // a vertex with too many neighbours for the walk positions
    if (vctl[0] == 0) break;
    if (vctl[1] == 0) { vec_ok = false; break; }                     // nothing moved although something waits: not on a verified state
  }
  if (st0 != L.vstate) HIPCHK(hipMemcpyAsync(L.vstate, st0, Vn, hipMemcpyDeviceToDevice, ctx->stream));   // final states in the first array
  d_vctl.reset();
  L.have_vec = vec_ok;
  HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
  Cnt flags{};
  HIPCHK(hipMemcpyAsync(&flags, s.cnt + 3, sizeof(Cnt), hipMemcpyDeviceToHost, ctx->stream));
  if (diff) HIPCHK(hipMemcpyAsync(diff->h_cnt, diff->cnt, sizeof(uint32_t) * mnav_map::kCounters, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->infl_steps = (uint32_t)(last.it < 0 ? 0 : last.it); ctx->infl_bands = last.bands; ctx->infl_evals = last.evals;
  ctx->infl_ms = ev_ms(ctx->ev[1], ctx->ev[3]); ctx->infl_ms_wave = ev_ms(ctx->ev[1], ctx->ev[2]);
  if (last.overflow) { ctx->err = "inflation wave did not converge (work-list overflow or step limit)"; return -1; }
  if (flags.n_next & kFlagWalkLimit) { ctx->err = "inflation wave: cascade-tree walk bound hit; the result may not be the reference's"; return -1; }
  if (flags.changed) { ctx->err = "inflation wave: the converged state is not a fixed point of the replay rule"; return -1; }
  L.ready = true;
  return 0;
}

int mnav_layer_inflation(mnav_ctx* ctx, uint32_t layer, uint32_t input_layer, double inflation_radius, double inscribed_radius,
                         double inscribed_value, double lethal_value, double cost_scaling_factor, const uint8_t* invalid)
{
  if (!ctx) return -1;
  ctx->err.clear();
  return layer_inflation_impl(ctx, layer, input_layer, inflation_radius, inscribed_radius, inscribed_value, lethal_value, cost_scaling_factor,
                              invalid, nullptr, nullptr);
}

int mnav_layer_download(mnav_ctx* ctx, uint32_t layer, float* costs_out, uint8_t* lethal_out, float* distances_out)
{
  if (!ctx) return -1;
  ctx->err.clear();
  if (layer >= ctx->layers.size() || !ctx->layers[layer].ready) { ctx->err = "layer is not resident"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  mnav_ctx::Layer& L = ctx->layers[layer];
  if (costs_out) HIPCHK(hipMemcpyAsync(costs_out, L.cost, sizeof(float) * ctx->V, hipMemcpyDeviceToHost, ctx->stream));
  if (lethal_out) HIPCHK(hipMemcpyAsync(lethal_out, L.lethal, ctx->V, hipMemcpyDeviceToHost, ctx->stream));
  if (distances_out) {
    if (!L.dist) { ctx->err = "this layer keeps no distances"; return -1; }
    HIPCHK(hipMemcpyAsync(distances_out, L.dist, sizeof(float) * ctx->V, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mnav_layer_download_vectors(mnav_ctx* ctx, uint32_t layer, float* vectors_out, uint8_t* has_vector_out)
{
  if (!ctx) return -1;
  ctx->err.clear();
  if (layer >= ctx->layers.size() || !ctx->layers[layer].ready) { ctx->err = "layer is not resident"; return -1; }
  mnav_ctx::Layer& L = ctx->layers[layer];
  if (!L.have_vec) { ctx->err = "this layer has no vector field (not an inflation layer, or a vertex with more than 15 neighbours)"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  const uint32_t V = ctx->V;
  if (vectors_out) HIPCHK(hipMemcpyAsync(vectors_out, L.vec, 12 * (size_t)V, hipMemcpyDeviceToHost, ctx->stream));
  std::vector<uint8_t> st(V ? V : 1);
  if (has_vector_out) HIPCHK(hipMemcpyAsync(st.data(), L.vstate, V, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (has_vector_out) for (uint32_t v = 0; v < V; ++v) has_vector_out[v] = st[v] == 1 ? 1 : 0;
  return 0;
}

int mnav_layer_stats(const mnav_ctx* ctx, uint32_t* steps, uint32_t* bands, uint64_t* evals, float* ms, uint32_t* verify_sweeps, float* ms_wave)
{
  if (!ctx) return -1;
  if (steps) *steps = ctx->infl_steps;
  if (bands) *bands = ctx->infl_bands;
  if (evals) *evals = ctx->infl_evals;
  if (ms) *ms = ctx->infl_ms;
  if (verify_sweeps) *verify_sweeps = ctx->verify_sweeps_used;
  if (ms_wave) *ms_wave = ctx->infl_ms_wave;
  return 0;
}

// CombinationLayer (max :44-85 / weighted sum :185-248) over resident layers, then MeshMap::computeEdgeWeights:
// the whole cost preparation of a map without a host copy of a single V-sized array.
int mnav_combine_layers(mnav_ctx* ctx, int mode, uint32_t n_layers, const uint32_t* layers, const float* weights, double edge_cost_factor,
                        const uint8_t* invalid)
{
  if (!ctx) return -1;
  ctx->err.clear();
  if (!ctx->have_mesh) { ctx->err = "mnav_upload_mesh has not been called"; return -1; }
  if (mode != 0 && mode != 1) { ctx->err = "combination mode must be 0 (max) or 1 (weighted sum)"; return -1; }
  if ((n_layers && !layers) || (mode == 1 && n_layers && !weights) || n_layers > 64) { ctx->err = "bad layer list"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  std::vector<const float*> ptrs(n_layers ? n_layers : 1, nullptr);
  for (uint32_t l = 0; l < n_layers; ++l) {
    if (layers[l] >= ctx->layers.size() || !ctx->layers[layers[l]].ready) { ctx->err = "layer is not resident"; return -1; }
    ptrs[l] = ctx->layers[layers[l]].cost;
  }
  ctx->rp.all = true;                                                // whole arrays replaced: a replan plans afresh, also after a failure half way
  if (ensure_edge_distances(ctx)) return -1;
  DevBuf<const float*> d_ptrs; DevBuf<float> d_wts;
  HIPCHK(d_ptrs.alloc(sizeof(float*) * (n_layers + 1)));
  HIPCHK(d_wts.alloc(sizeof(float) * (n_layers + 1)));
  int rc = 0;
  if (n_layers && hipMemcpyAsync(d_ptrs, ptrs.data(), sizeof(float*) * n_layers, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = -1;
  if (rc == 0 && mode == 1 && n_layers && hipMemcpyAsync(d_wts, weights, sizeof(float) * n_layers, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = -1;
  if (rc == 0 && ctx->d_cost.upload(ctx->stream, nullptr, ctx->V) != hipSuccess) { ctx->err = "cost buffer allocation failed"; rc = -1; }
  if (rc == 0) {
    const uint32_t gb = (ctx->V + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_combine_resident, dim3(gb ? gb : 1), dim3(kBlock), 0, ctx->stream, ctx->V, mode, n_layers, d_ptrs, d_wts, ctx->d_cost);
    if (hipGetLastError() != hipSuccess) rc = -1;
  }
  if (rc != 0 && ctx->err.empty()) ctx->err = "layer combination failed";
  if (rc == 0) rc = edge_weight_pass(ctx, edge_cost_factor, invalid, nullptr, nullptr);
  (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

// The incremental counterpart of mnav_combine_layers: CombinationLayer::onInputChanged + MeshMap::layerChanged +
// updateEdgeWeights(changed) for the n vertices a layer reported as changed (the layers themselves were updated on the
// device or re-uploaded before).  Same combination mode / layer list / weights as the full pass.
int mnav_combine_layers_update(mnav_ctx* ctx, int mode, uint32_t n_layers, const uint32_t* layers, const float* weights, uint32_t n,
                               const uint32_t* vertex_ids)
{
  if (!ctx) return -1;
  ctx->err.clear();
  if (!ctx->have_costs) { ctx->err = "no combined costs resident yet (mnav_combine_layers first)"; return -1; }
  if (mode != 0 && mode != 1) { ctx->err = "combination mode must be 0 (max) or 1 (weighted sum)"; return -1; }
  if ((n_layers && !layers) || (mode == 1 && n_layers && !weights) || n_layers > 64) { ctx->err = "bad layer list"; return -1; }
  if (n == 0) return 0;
  if (!vertex_ids) { ctx->err = "null id array"; return -1; }
  for (uint32_t i = 0; i < n; ++i) if (vertex_ids[i] >= ctx->V) { ctx->err = "vertex id out of range"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  std::vector<const float*> ptrs(n_layers ? n_layers : 1, nullptr);
  for (uint32_t l = 0; l < n_layers; ++l) {
    if (layers[l] >= ctx->layers.size() || !ctx->layers[layers[l]].ready) { ctx->err = "layer is not resident"; return -1; }
    ptrs[l] = ctx->layers[layers[l]].cost;
  }
  ctx->rp.all = true;                                                // (not one of the logging writers: a replan plans afresh)
  DevBuf<const float*> d_ptrs; DevBuf<float> d_wts, d_vals; DevBuf<uint32_t> d_ids;
  HIPCHK(d_ptrs.alloc(sizeof(float*) * (n_layers + 1)));
  HIPCHK(d_wts.alloc(sizeof(float) * (n_layers + 1)));
  HIPCHK(d_vals.alloc(sizeof(float) * n));
  HIPCHK(d_ids.alloc(sizeof(uint32_t) * n));
  std::vector<float> vals(n);
  int rc = 0;
  if (n_layers && hipMemcpyAsync(d_ptrs, ptrs.data(), sizeof(float*) * n_layers, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = -1;
  if (rc == 0 && mode == 1 && n_layers && hipMemcpyAsync(d_wts, weights, sizeof(float) * n_layers, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = -1;
  if (rc == 0 && hipMemcpyAsync(d_ids, vertex_ids, sizeof(uint32_t) * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = -1;
  if (rc == 0) {
    hipLaunchKernelGGL(k_combine_resident_ids, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, n, d_ids, mode, n_layers, d_ptrs, d_wts,
                       ctx->d_cost, d_vals);
    if (ctx->edge_cost_factor != 0.0)                               // "Edge costs are only affected by vertex costs if layer_factor is not 0" (:568-572)
      hipLaunchKernelGGL(k_update_edge_weights, dim3((8 * n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, n, d_ids, ctx->d_row_ptr,
                         ctx->d_nbr_u, ctx->d_nbr_e, ctx->d_edge_dist, ctx->d_cost, ctx->edge_cost_factor, ctx->d_w);
    if (hipGetLastError() != hipSuccess) rc = -1;
  }
  if (rc == 0 && hipMemcpyAsync(vals.data(), d_vals, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = -1;
  (void)hipStreamSynchronize(ctx->stream);
  if (rc != 0) { if (ctx->err.empty()) ctx->err = "incremental combination failed"; return rc; }
  for (uint32_t i = 0; i < n; ++i) ctx->h_cost[vertex_ids[i]] = vals[i];
  ctx->nbr_valid = ctx->crn_valid = false;                          // the cost-limit folded copies are rebuilt on the next plan
  return 0;
}

// The tail of a Dijkstra call whose engine (and, unless the call is paths-only, finalize pass) has run: vertex paths, result
// records, the vector map, the downloads and the statistics of m device plans; map: device plan -> caller's index.
// sub (the per-plan replan, finalized plans only): the m plans are those of compacted tables -- the first n_vec of them get a
// vector map, the rest (fields nobody rewound) have their settled vertices counted, and plan k lives in slot sub->slot[k].
// Returns 0 or -1 (ctx->err set).
struct TailSub { const Plan* plans; PlanResult* res; float* const* vecptrs; uint32_t n_vec; const uint32_t* slot; };
static int dijkstra_tail(mnav_ctx* ctx, uint32_t m, int engine, const std::vector<uint32_t>& map, std::vector<uint32_t>& codes, float* dist_out,
                         uint32_t* pred_out, uint32_t* path_out, uint32_t path_cap, uint32_t* path_len, float* vecmap_out, bool want_vecmap,
                         const TailSub* sub = nullptr)
{
  const uint32_t V = ctx->V;
  const Plan* const d_plans = sub ? sub->plans : ctx->d_plans.get();
  PlanResult* const d_res = sub ? sub->res : ctx->d_res.get();
  const uint32_t n_vec = sub ? sub->n_vec : m;
  const PathRows rows1{ ctx->d_paths, ctx->path_stride, nullptr, nullptr };
  PathRows rows2{ nullptr, 0u, nullptr, nullptr };
  const uint32_t gc = (V + kBlock * 4 - 1) / (kBlock * 4);
  if (engine == 5 && ctx->lazy_paths) {
    hipLaunchKernelGGL(k_tb_path, dim3(m), dim3(kWave), 0, ctx->stream, ctx->tb_args, ctx->d_row_ptr, ctx->d_nbr, V, ctx->d_res, rows1, ctx->d_mismatch);
    ctx->tb.count_pending = true;                                  // settled vertices (a statistic): counted when somebody asks, mnav_get_stats
  } else if (ctx->lazy_paths) {
    hipLaunchKernelGGL(k_path_lazy, dim3(m), dim3(kWave), 0, ctx->stream, ctx->d_plans, ctx->d_tplans, ctx->d_res, rows1, ctx->d_mismatch);
    hipLaunchKernelGGL(k_count_goal, dim3(gc ? gc : 1, m), dim3(kBlock), 0, ctx->stream, ctx->d_plans, ctx->d_res);
  } else
  hipLaunchKernelGGL(k_finish<kPlannerDijkstra>, dim3(m), dim3(64), 0, ctx->stream, d_plans, d_res, rows1);
  if (engine == 1)   // the tile engines count the settled vertices in k_dij_finalize
    hipLaunchKernelGGL(k_count, dim3(gc ? gc : 1, m), dim3(kBlock), 0, ctx->stream, d_plans, d_res);
  if (sub && m > n_vec)
    hipLaunchKernelGGL(k_count, dim3(gc ? gc : 1, m - n_vec), dim3(kBlock), 0, ctx->stream, d_plans + n_vec, d_res + n_vec);
  (void)hipEventRecord(ctx->ev[4], ctx->stream);
  if (want_vecmap && n_vec && !(engine == 5 && !ctx->lazy_paths))   // (the tile-batch engine's finalize pass writes the vector map itself)
    hipLaunchKernelGGL(k_vecmap_dijkstra, dim3(gc ? gc : 1, n_vec), dim3(kBlock), 0, ctx->stream, d_plans, ctx->d_xyz, sub ? sub->vecptrs : ctx->d_vecptrs.get());
  (void)hipEventRecord(ctx->ev[5], ctx->stream);
  // The packed paths follow the walk on the device: offsets by k_pack_offsets, k_pack_paths behind it, nothing in between that
  // waits for the host (until this was moved the lengths went down, the host summed them and sent the offsets up again, with
  // the device idle meanwhile).  The pack buffer holds the worst case, every row full.
  const bool pack = path_out && path_cap;
  auto ensure_pack = [&](size_t words) {
    if (ctx->pack_words < words) {
      ctx->d_pack.reset(); ctx->pack_words = 0;
      if (ctx->d_pack.alloc(4 * words) != hipSuccess) return false;
      ctx->pack_words = words;
    }
    if (ctx->pack_meta_n < 2 * (size_t)m) {
      ctx->pack_meta_n = 0;
      if (ctx->d_pack_meta.alloc(4 * 2 * (size_t)m) != hipSuccess) return false;
      ctx->pack_meta_n = 2 * (size_t)m;
    }
    return true;
  };
  if (pack) {
    if (!ensure_pack((size_t)m * (ctx->path_stride ? ctx->path_stride : 1u))) { ctx->err = "path buffers: out of memory"; return -1; }
    hipLaunchKernelGGL(k_pack_offsets, dim3(1), dim3(1024), 0, ctx->stream, d_res, m, ctx->d_pack_meta, ctx->d_pack_meta + m);
    hipLaunchKernelGGL(k_pack_paths, dim3(m), dim3(kBlock), 0, ctx->stream, rows1, rows2, ctx->d_pack_meta, ctx->d_pack_meta + m, ctx->d_pack);
  }
  const bool check_mism = ctx->last_engine != 1;
  if (check_mism && !ctx->h_mism && ctx->h_mism.alloc(4) != hipSuccess) { ctx->err = "result download failed"; return -1; }
  if (hipMemcpyAsync(ctx->h_res, d_res, sizeof(PlanResult) * m, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      (check_mism && hipMemcpyAsync(ctx->h_mism, ctx->d_mismatch, 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->err = "result download failed"; return -1; }
  bool repack = false;
  {
    // paths longer than the default rows (corridors, mazes): ONLY those plans are walked again, into rows of exactly their
    // length (the first walk counted it) in one packed buffer, and all paths are packed again with offsets from the host
    size_t over_words = 0;
    std::vector<unsigned long long> ooff(m, 0ull); std::vector<uint32_t> ocap(m, 0u);
    for (uint32_t k = 0; k < m; ++k)
      if (ctx->h_res[k].code == kPathOverflow) { ooff[k] = over_words; ocap[k] = ctx->h_res[k].path_len; over_words += ctx->h_res[k].path_len; }
    if (over_words) {
      std::vector<PlanResult> keep(ctx->h_res.get(), ctx->h_res + m);   // settled / evals were accumulated by other kernels
      ctx->d_over.reset(); ctx->d_over_off.reset(); ctx->d_over_cap.reset();
      if (ctx->d_over.alloc(4 * over_words) != hipSuccess || ctx->d_over_off.alloc(8 * (size_t)m) != hipSuccess || ctx->d_over_cap.alloc(4 * (size_t)m) != hipSuccess ||
          hipMemcpyAsync(ctx->d_over_off, ooff.data(), 8 * (size_t)m, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
          hipMemcpyAsync(ctx->d_over_cap, ocap.data(), 4 * (size_t)m, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        { ctx->err = "path buffers: out of memory"; return -1; }
      rows2 = PathRows{ ctx->d_over, 0u, ctx->d_over_off, ctx->d_over_cap };
      if (engine == 5 && ctx->lazy_paths) hipLaunchKernelGGL(k_tb_path, dim3(m), dim3(kWave), 0, ctx->stream, ctx->tb_args, ctx->d_row_ptr, ctx->d_nbr, V, ctx->d_res, rows2, ctx->d_mismatch);
      else if (ctx->lazy_paths) hipLaunchKernelGGL(k_path_lazy, dim3(m), dim3(kWave), 0, ctx->stream, ctx->d_plans, ctx->d_tplans, ctx->d_res, rows2, ctx->d_mismatch);
      else hipLaunchKernelGGL(k_finish<kPlannerDijkstra>, dim3(m), dim3(64), 0, ctx->stream, d_plans, d_res, rows2);
      if (hipMemcpyAsync(ctx->h_res, d_res, sizeof(PlanResult) * m, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
          (check_mism && hipMemcpyAsync(ctx->h_mism, ctx->d_mismatch, 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) ||
          hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->err = "result download failed"; return -1; }
      for (uint32_t k = 0; k < m; ++k) ctx->h_res[k].settled = keep[k].settled;
      repack = true;
    }
  }
  if (check_mism && *ctx->h_mism != 0u) {
    ctx->err = "tiled SSSP did not reach its fixed point (" + std::to_string(*ctx->h_mism) + " vertices)";
    return -1;
  }
  MTRACE("results downloaded");
  // all vertex paths: packed and reversed on the device (k_pack_paths), one dense copy into a pinned buffer -- of the words
  // the downloaded lengths add up to, which is why this copy comes after the results and not with them (rows are sized
  // for paths an order of magnitude longer than a terrain's, so the row-full worst case is many times these words)
  std::vector<uint32_t> offs(m + 1, 0), lens(m, 0);
  for (uint32_t k = 0; k < m; ++k) {
    lens[k] = (ctx->h_res[k].code == MNAV_SUCCESS) ? ctx->h_res[k].path_len : 0u;
    offs[k + 1] = offs[k] + lens[k];
  }
  const size_t total = offs[m];
  if (total && pack) {
    if (ctx->h_pack_words < total) {
      ctx->h_pack.reset(); ctx->h_pack_words = 0;
      const size_t want = total + total / 4 + 1024;
      if (ctx->h_pack.alloc(4 * want) != hipSuccess) { ctx->err = "path buffers: out of memory"; return -1; }
      ctx->h_pack_words = want;
    }
    if (repack) {
      if (!ensure_pack(total)) { ctx->err = "path buffers: out of memory"; return -1; }
      if (hipMemcpyAsync(ctx->d_pack_meta, offs.data(), 4 * (size_t)m, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
          hipMemcpyAsync(ctx->d_pack_meta + m, lens.data(), 4 * (size_t)m, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        { ctx->err = "path download failed"; return -1; }
      hipLaunchKernelGGL(k_pack_paths, dim3(m), dim3(kBlock), 0, ctx->stream, rows1, rows2, ctx->d_pack_meta, ctx->d_pack_meta + m, ctx->d_pack);
    }
    if (hipMemcpyAsync(ctx->h_pack, ctx->d_pack, 4 * total, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) { ctx->err = "path download failed"; return -1; }
  }
  // The tile-batch engine's other distance buffer is cleaned for the next call from HERE (tb_clean_other: its stream waits for an
  // event recorded at this point), under the host's copy-out below and the gap before the next call.  Not earlier: launched
  // behind k_pack_paths, the fill held the download of the results back until it had finished (6.6 - 7.2 ms for a copy of
  // microseconds, profiles/sched_pass_kernel_stats.md) -- the copy is a kernel too, and a kernel next to the fill ends with it.
  // (A call that downloads V-sized outputs below cleans behind those instead.)
  const bool field_downloads = dist_out || pred_out || (vecmap_out && want_vecmap);
  if (engine == 5 && !field_downloads && tb_clean_other(ctx)) return -1;
  if (total && pack && hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->err = "path download failed"; return -1; }
  MTRACE("paths downloaded");
  for (uint32_t k = 0; k < m; ++k) {
    const uint32_t i = map[k];
    const PlanResult& r = ctx->h_res[k];
    const Slot& sl = ctx->slots[sub ? sub->slot[k] : k];
    codes[i] = r.code;
    if (r.code == MNAV_SUCCESS) {
      if (path_len) path_len[i] = r.path_len;
      if (path_out && path_cap && r.path_len)                         // reference list order: seed ... pred[target]
        memcpy(path_out + (size_t)i * path_cap, ctx->h_pack + offs[k], 4 * (size_t)std::min(r.path_len, path_cap));
    }
    if (dist_out && hipMemcpyAsync(dist_out + (size_t)i * V, sl.dist, 4 * (size_t)V, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
      { ctx->err = "dist download failed"; return -1; }
    if (pred_out && hipMemcpyAsync(pred_out + (size_t)i * V, sl.pred, 4 * (size_t)V, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
      { ctx->err = "pred download failed"; return -1; }
    if (vecmap_out && want_vecmap && hipMemcpyAsync(vecmap_out + (size_t)i * 3 * V, sl.vecmap, 12 * (size_t)V, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
      { ctx->err = "vecmap download failed"; return -1; }
  }
  MTRACE("paths copied out");
  (void)hipEventRecord(ctx->ev[6], ctx->stream);
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->err = "sync failed"; return -1; }
  if (engine == 5 && tb_clean_other(ctx)) return -1;   // (does nothing when the buffer was cleaned above)
  finish_stats(ctx, m, false);
  MTRACE("stats done");
  return 0;
}

// The engine `auto` picks for m plans of a Dijkstra call: 0 tile rounds, 5 tile-batch, 6 asynchronous tiles.
static int dijkstra_auto_engine(mnav_ctx* ctx, uint32_t m0)
{
  // The tile-batch engine advances all plans tile by tile, 16 plans per quarter of a wave (k_tb_solve_q).  Its floor is one
  // stream pass per iteration (~190 iterations x ~180 us on the 1M mesh, ~600 x 300 us at 10M), whatever the batch; above
  // that it beats the per-plan engines at every size measured (round 4, plans/s, tiled / persistent / tile-batch --
  // 1M: 64 plans 1084 / 496 / 1359, 256: 1879 / 1929 / 4392, 1024: 2223 / 7107 / 12871;
  // 10M: 64 plans 196 / 41 / 189, 256: 252 / 163 / 409, 1024: 254 / 594 / 924).
  const double tiles = std::max(1.0, (double)ctx->V / (0.9 * ctx->tb.T));
  const bool fills = m0 >= ctx->tb.min_batch && m0 <= 65535u && (double)m0 >= tiles / 1000.0;
  // Below that: the asynchronous tile engine (mnav_async.h: one launch, per-plan ticket queues of woken tiles; what a real
  // makePlan call -- ONE plan -- runs on), up to async_max_batch plans.  Measured round 5, ms per call on the 1M mesh, rounds /
  // tile-batch / asynchronous: 1 plan 10.1 / 20 / 6.8, 8 plans 28 / 29 / 9.7, 47 plans 55 / 38 / 22.9, 64 plans 65 / 46 / 27.5
  // (10M mesh: 8 plans 83 / - / 45, 47 plans 243 / - / 182, 64 plans 330 / 340 / 224); it grows linearly with the batch
  // where the tile-batch engine's iterations are shared by all plans: the engines cross at about a hundred plans.
  // Round 6 (a ticket's round trips cut, mnav_async.h): ms per call, asynchronous / tile-batch, 1M mesh 96 plans 29 / 51,
  // 128: 36 / 53, 192: 52 / 58, 256: 69 / 60; 10M mesh 96: 261 / 343, 128: 325 / 388, 192: 540 / 470
  // (profiles/r06_async_crossover.json): the engines now cross at about 160 plans on both meshes.
  return (m0 <= opt_u32(ctx->opt.async_max_batch, 160u)) ? 6 : fills ? 5 : 0;
}

// The plans of a batch in the order their engine wants them (results are mapped back through `map`).
static int dijkstra_order(mnav_ctx* ctx, int engine, std::vector<PlanIn>& in, std::vector<uint32_t>& map)
{
  const uint32_t V = ctx->V;
  if (engine == 5 && in.size() > 1) {
    // plans whose waves start close to each other are neighbours in the batch: their slices of a tile are adjacent in memory
    // and they tend to have work on the same tiles at the same time
    if (tb_build(ctx)) return -1;
    std::vector<uint32_t> ord(in.size());
    std::iota(ord.begin(), ord.end(), 0u);
    const std::vector<uint32_t>& vt = ctx->tb.vert_tile;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return vt[in[x].seed[0]] < vt[in[y].seed[0]]; });
    std::vector<PlanIn> in2(in.size()); std::vector<uint32_t> map2(in.size());
    for (size_t i = 0; i < in.size(); ++i) { in2[i] = in[ord[i]]; map2[i] = map[ord[i]]; }
    in.swap(in2); map.swap(map2);
  } else
  if (in.size() > 1 && ctx->h_xyz.size() == 3 * (size_t)V) {
    std::vector<uint32_t> ord(in.size());
    std::iota(ord.begin(), ord.end(), 0u);
    std::vector<float> est(in.size());
    for (size_t i = 0; i < in.size(); ++i) {
      const float* a = &ctx->h_xyz[3 * (size_t)in[i].seed[0]];
      const float* b = &ctx->h_xyz[3 * (size_t)in[i].target[0]];
      est[i] = (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
    }
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return est[x] > est[y]; });
    std::vector<PlanIn> in2(in.size()); std::vector<uint32_t> map2(in.size());
    for (size_t i = 0; i < in.size(); ++i) { in2[i] = in[ord[i]]; map2[i] = map[ord[i]]; }
    in.swap(in2); map.swap(map2);
  }
  return 0;
}

// The engine run of m plans in the first m slots.  Returns 0, -1 (error) or 1 (cancelled); nothing of a failed or cancelled
// call stays in flight.  *engine: what ran (the asynchronous engine hands a call it cannot finish to the tile rounds).
static int dijkstra_dispatch(mnav_ctx* ctx, uint32_t m, const std::vector<PlanIn>& in, double offset, bool engine_auto, int* engine_io)
{
  int engine = *engine_io;
  const bool want_path = true;
  int rc = (engine == 0) ? run_dijkstra_tiled(ctx, m, in, offset)
         : (engine == 6) ? run_dijkstra_async(ctx, m, in, offset)
         : (engine == 5) ? run_dijkstra_tb(ctx, m, in, offset)
                         : run_plans<kPlannerDijkstra>(ctx, m, in, offset, want_path);
  // ticket ring exhausted: the rounds start over.  So they do when the in-kernel watchdog gave up (rc 3) on an engine that `auto`
  // picked: the rounds have the whole max_wall_s (a serialising profiler, a mesh far beyond the tuned sizes)
  if (engine == 6 && (rc == 2 || (rc == 3 && engine_auto))) { ctx->err.clear(); engine = 0; rc = run_dijkstra_tiled(ctx, m, in, offset); }
  if (rc == 3) rc = -1;
  MTRACE("engine returned");
  if (rc != 0) (void)hipStreamSynchronize(ctx->stream);             // nothing of a failed / cancelled call stays in flight
  *engine_io = engine;
  return rc;
}

static uint32_t dijkstra_impl(mnav_ctx* ctx, uint32_t n, const uint32_t* seeds, const uint32_t* targets, double offset,
                              double cost_limit, uint32_t* codes_out, float* dist_out, uint32_t* pred_out, uint32_t* path_out,
                              uint32_t path_cap, uint32_t* path_len, float* vecmap_out, bool want_vecmap)
{
  if (check_ready(ctx)) return MNAV_INTERNAL_ERROR;
  ctx->err.clear();
  // goal_dist = dist[target] + offset cuts the wave off BEHIND the robot (dijkstra :296).  A negative offset (the reference
  // takes any double) stops the expansion AT the robot vertex: the engines run with the bound of offset 0 -- everything at or
  // below dist[target] is final then -- and the passes that derive tentative values, predecessors and paths apply the
  // reference's expanded set through goal_cut() (mnav_eval.h).
  if (offset != offset) { ctx->err = "goal_dist_offset is NaN"; return MNAV_INTERNAL_ERROR; }
  cancel_reset(ctx);
  want_vecmap = want_vecmap || ctx->resident_vecmap;
  ctx->want_vec = want_vecmap;
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MNAV_INTERNAL_ERROR; }
  MTRACE("start");
  const uint32_t V = ctx->V;
  uint32_t worst = MNAV_SUCCESS;
  ctx->res.record_dijkstra(n, seeds, targets, cost_limit, offset);   // what a replan needs of this call; its fields count once it has gone through
  // id checks stand in for the optional-handle tests of dijkstra :240-243
  std::vector<PlanIn> in; std::vector<uint32_t> map;   // map: device plan -> caller index
  std::vector<uint32_t> codes(n, MNAV_SUCCESS);
  std::vector<uint8_t> cleared(n, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (path_len) path_len[i] = 0;
    if (seeds[i] >= V) { codes[i] = MNAV_INVALID_START; continue; }
    if (targets[i] >= V) { codes[i] = MNAV_INVALID_GOAL; continue; }
    if (seeds[i] == targets[i]) { cleared[i] = 1; continue; }   // :252-255 SUCCESS right after clearing the maps
    in.push_back(vertex_plan(seeds[i], targets[i])); map.push_back(i);
  }
  // Longest plans first: a plan's work grows with the area its wave sweeps before it reaches the robot
  // vertex, i.e. with the squared seed-target distance.  Workgroups are dispatched in plan order, so when a
  // batch holds more plans than the device runs at once the short ones back-fill behind the long ones
  // instead of leaving a tail (results are mapped back through `map`).
  // engine: 0 = tiled rounds, 1 = band steps, 3 = auto, 5 = tile-batch (plan-vectorised, large batches), 6 = asynchronous tiles
  int engine = ctx->dij_engine;
  const bool engine_auto = engine == 3;
  // paths only (nothing V-sized asked for, nothing kept resident): no finalize pass, predecessors along the path only
  ctx->lazy_paths = ctx->allow_lazy_paths && !dist_out && !pred_out && !want_vecmap && !ctx->resident_vecmap;
  {
    const uint32_t m0 = (uint32_t)in.size();
    // auto: one wave per (tile, 64 plans) for large batches, one workgroup per plan for medium ones, tile rounds otherwise
    if (engine == 3) engine = dijkstra_auto_engine(ctx, m0);
    if (engine == 5 && m0 > 65535u) engine = 0;                       // (plan ids are 16 bits in the tile-batch buckets)
    if (engine == 1 && offset < 0.0) engine = 0;                      // the band steps arm goal_dist inside the loop: tile rounds for a negative offset
  }
  if (dijkstra_order(ctx, engine, in, map)) return MNAV_INTERNAL_ERROR;
  const Resident::FinalizeClaim held = ctx->res.take_finalize_claim();   // what the last finalize pass of the tile-batch engine left in the slots (this call's to use, nobody's after)
  ctx->res.outputs_begin(Resident::kDijkstra, n, map);               // outputs of the previous call are gone; this call's once it has gone through:
  resident_outputs_begin(ctx);                                        // every error return below leaves none
  (void)hipEventRecord(ctx->ev[0], ctx->stream);
  const uint32_t m = (uint32_t)in.size();
  if (m) {
    if (materialize(ctx, false, cost_limit)) return MNAV_INTERNAL_ERROR;
    ctx->tb.claim_np = held.slots; ctx->tb.claim_vec = held.vecmaps;   // (run_dijkstra_tb takes it; good for this dispatch only)
    const int rc = dijkstra_dispatch(ctx, m, in, offset, engine_auto, &engine);
    ctx->tb.claim_np = 0;
    if (rc < 0) return MNAV_INTERNAL_ERROR;
    if (rc == 1) { for (uint32_t i = 0; i < n; ++i) if (codes_out) codes_out[i] = MNAV_CANCELED; return MNAV_CANCELED; }   // :350-354
    ctx->last_engine = engine;
    if (engine == 1) ctx->lazy_paths = false;                         // the band steps keep their predecessors as they go
    if (dijkstra_tail(ctx, m, engine, map, codes, dist_out, pred_out, path_out, path_cap, path_len, vecmap_out, want_vecmap)) return MNAV_INTERNAL_ERROR;
  }
  ctx->res.commit_dijkstra(engine, m, ctx->lazy_paths, want_vecmap);
  resident_outputs_commit(ctx);
  // plans rejected before reaching the device: the reference has cleared its maps by then
  for (uint32_t i = 0; i < n; ++i) {
    if (codes[i] == MNAV_INVALID_START || codes[i] == MNAV_INVALID_GOAL || cleared[i]) {
      if (dist_out) for (uint32_t v = 0; v < V; ++v) dist_out[(size_t)i * V + v] = INFINITY;
      if (pred_out) for (uint32_t v = 0; v < V; ++v) pred_out[(size_t)i * V + v] = v;
    }
    if (codes_out) codes_out[i] = codes[i];
    if (codes[i] != MNAV_SUCCESS && worst == MNAV_SUCCESS) worst = codes[i];
  }
  return worst;
}

uint32_t mnav_plan_dijkstra(mnav_ctx* ctx, uint32_t seed_vertex, uint32_t target_vertex, double goal_dist_offset, double cost_limit,
                            float* dist_out, uint32_t* pred_out, uint32_t* path_out, uint32_t path_cap, uint32_t* path_len,
                            float* vecmap_out)
{
  if (!ctx) return MNAV_INTERNAL_ERROR;
  uint32_t code = MNAV_INTERNAL_ERROR;
  uint32_t len = 0;
  const uint32_t rc = dijkstra_impl(ctx, 1, &seed_vertex, &target_vertex, goal_dist_offset, cost_limit, &code, dist_out, pred_out,
                                    path_out, path_cap, &len, vecmap_out, true);
  if (path_len) *path_len = len;
  return rc == MNAV_INTERNAL_ERROR || rc == MNAV_CANCELED ? rc : code;
}

uint32_t mnav_plan_dijkstra_batch(mnav_ctx* ctx, uint32_t n, const uint32_t* seeds, const uint32_t* targets, double goal_dist_offset,
                                  double cost_limit, uint32_t* codes_out, float* dist_out, uint32_t* pred_out, uint32_t* path_out,
                                  uint32_t path_cap, uint32_t* path_len)
{
  if (!ctx) return MNAV_INTERNAL_ERROR;
  if (n == 0) return MNAV_SUCCESS;
  if (!seeds || !targets) { ctx->err = "null seeds/targets"; return MNAV_INTERNAL_ERROR; }
  return dijkstra_impl(ctx, n, seeds, targets, goal_dist_offset, cost_limit, codes_out, dist_out, pred_out, path_out, path_cap,
                       path_len, nullptr, false);
}

static uint32_t cvp_impl(mnav_ctx* ctx, uint32_t n, const float* seed_pos, const uint32_t* seed_faces, const uint32_t* target_faces,
                         double goal_dist_offset, double cost_limit, uint32_t* codes_out, float* dist_out, uint32_t* pred_out,
                         float* direction_out, uint32_t* cutface_out, float* vecmap_out)
{
  if (check_ready(ctx)) return MNAV_INTERNAL_ERROR;
  ctx->err.clear();
  if (goal_dist_offset != goal_dist_offset) { ctx->err = "goal_dist_offset is NaN"; return MNAV_INTERNAL_ERROR; }   // any double otherwise: a negative one
                                                                                                                      // stops the wave at the arming pop (passes_goal_cut)
  cancel_reset(ctx);
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MNAV_INTERNAL_ERROR; }
  const uint32_t V = ctx->V;
  if (!ctx->have_normals) { ctx->err = "vertex normals were not uploaded"; return MNAV_INTERNAL_ERROR; }
  if (V > (1u << kKeyIdBits)) { ctx->err = "CVP pop keys hold 26-bit vertex ids: mesh too large"; return MNAV_INTERNAL_ERROR; }
  std::vector<uint32_t> codes(n, MNAV_SUCCESS), map;
  std::vector<PlanIn> in;
  std::vector<float> sp;
  for (uint32_t i = 0; i < n; ++i) {
    if (seed_faces[i] >= ctx->F) { codes[i] = MNAV_INVALID_START; continue; }      // cvp :681-685
    if (target_faces[i] >= ctx->F) { codes[i] = MNAV_INVALID_GOAL; continue; }     // cvp :686-690
    PlanIn p{};
    for (int k = 0; k < 3; ++k) {
      p.seed[k] = ctx->h_faces[3 * (size_t)seed_faces[i] + k];
      p.target[k] = ctx->h_faces[3 * (size_t)target_faces[i] + k];
    }
    for (int k = 0; k < 3; ++k) {
      // cvp :721-723  diff = start - vertex; dist = diff.length()  (float arithmetic)
      const float dx = seed_pos[3 * (size_t)i] - ctx->h_xyz[3 * (size_t)p.seed[k]];
      const float dy = seed_pos[3 * (size_t)i + 1] - ctx->h_xyz[3 * (size_t)p.seed[k] + 1];
      const float dz = seed_pos[3 * (size_t)i + 2] - ctx->h_xyz[3 * (size_t)p.seed[k] + 2];
      const float l2 = dx * dx + dy * dy + dz * dz;
      p.seed_d[k] = sqrtf(l2);
      p.seed_expands[k] = (!((double)ctx->h_cost[p.seed[k]] >= cost_limit) && !ctx->h_invalid[p.seed[k]]) ? 1u : 0u;       // cvp :757,760
      p.target_expands[k] = (!((double)ctx->h_cost[p.target[k]] >= cost_limit) && !ctx->h_invalid[p.target[k]]) ? 1u : 0u;
    }
    p.seed_face = seed_faces[i];
    in.push_back(p); map.push_back(i);
    sp.insert(sp.end(), seed_pos + 3 * (size_t)i, seed_pos + 3 * (size_t)i + 3);
  }
  const uint32_t m = (uint32_t)in.size();
  ctx->res.outputs_begin(Resident::kCvp, n, map);                    // the slots' dist now holds CVP potentials: nothing a replan can rewind.
  resident_outputs_begin(ctx);                                        // (As found: the recorded Dijkstra call survives -- a replan then plans it afresh, reason 1)
  (void)hipEventRecord(ctx->ev[0], ctx->stream);
  ctx->last_engine = 1;
  uint32_t worst = MNAV_SUCCESS;
  if (m) {
    if (materialize(ctx, true, cost_limit)) return MNAV_INTERNAL_ERROR;
    if (ctx->seed_pos_cap < m) {
      if (ctx->d_seed_pos.alloc(12 * (size_t)m) != hipSuccess) { ctx->err = "alloc failed"; return MNAV_INTERNAL_ERROR; }
      ctx->seed_pos_cap = m;
    }
    if (hipMemcpyAsync(ctx->d_seed_pos, sp.data(), 12 * (size_t)m, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
      { ctx->err = "seed upload failed"; return MNAV_INTERNAL_ERROR; }
    const int rc = run_plans<kPlannerCvp>(ctx, m, in, goal_dist_offset, false);
    if (rc != 0) (void)hipStreamSynchronize(ctx->stream);
    if (rc < 0) return MNAV_INTERNAL_ERROR;
    if (rc == 1) { if (codes_out) for (uint32_t i = 0; i < n; ++i) codes_out[i] = MNAV_CANCELED; return MNAV_CANCELED; }   // cvp :888-892
    ctx->res.commit_cvp(m);
    hipLaunchKernelGGL(k_finish<kPlannerCvp>, dim3(m), dim3(64), 0, ctx->stream, ctx->d_plans, ctx->d_res, PathRows{ nullptr, 0u, nullptr, nullptr });
    const uint32_t gc = (V + kBlock * 4 - 1) / (kBlock * 4);
    hipLaunchKernelGGL(k_count, dim3(gc ? gc : 1, m), dim3(kBlock), 0, ctx->stream, ctx->d_plans, ctx->d_res);
    (void)hipEventRecord(ctx->ev[4], ctx->stream);
    hipLaunchKernelGGL(k_vecmap_cvp, dim3(gc ? gc : 1, m), dim3(kBlock), 0, ctx->stream, ctx->d_plans, ctx->d_xyz, ctx->d_nrm,
                       ctx->d_vecptrs, ctx->d_seed_pos);                // cvp :897
    (void)hipEventRecord(ctx->ev[5], ctx->stream);
    bool ok = hipMemcpyAsync(ctx->h_res, ctx->d_res, sizeof(PlanResult) * m, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
    for (uint32_t k = 0; k < m && ok; ++k) {
      const uint32_t i = map[k];
      Slot& s = ctx->slots[k];
      if (ok && dist_out) ok = hipMemcpyAsync(dist_out + (size_t)i * V, s.dist, 4 * (size_t)V, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
      if (ok && pred_out) ok = hipMemcpyAsync(pred_out + (size_t)i * V, s.pred, 4 * (size_t)V, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
      if (ok && direction_out) ok = hipMemcpyAsync(direction_out + (size_t)i * V, s.dirn, 4 * (size_t)V, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
      if (ok && cutface_out) ok = hipMemcpyAsync(cutface_out + (size_t)i * V, s.cutf, 4 * (size_t)V, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
      if (ok && vecmap_out) ok = hipMemcpyAsync(vecmap_out + (size_t)i * 3 * V, s.vecmap, 12 * (size_t)V, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
    }
    (void)hipEventRecord(ctx->ev[6], ctx->stream);
    if (!ok || hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->err = "output download failed"; return MNAV_INTERNAL_ERROR; }
    finish_stats(ctx, m, true);
    for (uint32_t k = 0; k < m; ++k) {
      codes[map[k]] = ctx->h_res[k].code;
      if (ctx->h_res[k].code == MNAV_INTERNAL_ERROR) {
        const uint32_t o = ctx->h_res[k].overflow;
        ctx->err = (o & 8u) ? "CVP: a walk over the cascade tree hit its bound on the converged state (pop order not guaranteed)"
                 : (o & 16u) ? "CVP: verification sweep found a vertex that is not a fixed point of the gather rule"
                             : "CVP wavefront did not converge (step cap)";
      }
    }
  }
  for (uint32_t i = 0; i < n; ++i) {
    if (codes_out) codes_out[i] = codes[i];
    if (codes[i] != MNAV_SUCCESS && worst == MNAV_SUCCESS) worst = codes[i];
  }
  return worst;
}

uint32_t mnav_plan_cvp(mnav_ctx* ctx, const float seed_pos[3], uint32_t seed_face, uint32_t target_face, double goal_dist_offset,
                       double cost_limit, float* dist_out, uint32_t* pred_out, float* direction_out, uint32_t* cutface_out,
                       float* vecmap_out)
{
  if (!ctx) return MNAV_INTERNAL_ERROR;
  if (!seed_pos) return MNAV_INVALID_START;
  uint32_t code = MNAV_INTERNAL_ERROR;
  const uint32_t rc = cvp_impl(ctx, 1, seed_pos, &seed_face, &target_face, goal_dist_offset, cost_limit, &code, dist_out, pred_out,
                               direction_out, cutface_out, vecmap_out);
  return (rc == MNAV_INTERNAL_ERROR || rc == MNAV_CANCELED) ? rc : code;
}

uint32_t mnav_plan_cvp_batch(mnav_ctx* ctx, uint32_t n, const float* seed_pos, const uint32_t* seed_faces, const uint32_t* target_faces,
                             double goal_dist_offset, double cost_limit, uint32_t* codes_out, float* dist_out, uint32_t* pred_out,
                             float* vecmap_out)
{
  if (!ctx) return MNAV_INTERNAL_ERROR;
  if (n == 0) return MNAV_SUCCESS;
  if (!seed_pos || !seed_faces || !target_faces) { ctx->err = "null seeds/targets"; return MNAV_INTERNAL_ERROR; }
  return cvp_impl(ctx, n, seed_pos, seed_faces, target_faces, goal_dist_offset, cost_limit, codes_out, dist_out, pred_out, nullptr, nullptr,
                  vecmap_out);
}

#include "mnav_shard_capi.h"   // mnav_shard_* (one plan over several GPUs)
#include "mnav_obstacle_capi.h"   // mnav_layer_obstacle, mnav_obstacle_stats
#include "mnav_nbhd_capi.h"       // mnav_layer_height_diff / _roughness / _ridge, mnav_neighbourhood_stats
#include "mnav_clearance_capi.h"  // mnav_layer_clearance, mnav_layer_border, mnav_clearance_download, mnav_clearance_stats
#include "mnav_locate_capi.h"     // mnav_locate, mnav_locate_stats, mnav_plan_dijkstra_batch_at, mnav_plan_cvp_batch_at
#include "mnav_follow_capi.h"     // mnav_follow_batch, mnav_follow_stats
#include "mnav_rollout_capi.h"    // mnav_follow_rollout, mnav_rollout_stats, mnav_fleet_rollout, mnav_fleet_rollout_stats, mnav_fleet_rollout_yield, mnav_fleet_yield_stats, mnav_fleet_rollout_rings, mnav_fleet_ring_stats
#include "mnav_sample_capi.h"     // mnav_follow_sample, mnav_sample_stats
#include "mnav_graph_capi.h"      // mnav_map_configure / _compute / _layer_changed / _update_layer / _obstacle / _stats
#include "mnav_replan_capi.h"     // mnav_replan_dijkstra_batch, mnav_replan_stats
#include "mnav_replan_each_capi.h"   // mnav_replan_dijkstra_each, mnav_replan_each_stats
#include "mnav_fleet_capi.h"      // mnav_fleet_paths, mnav_fleet_walks, mnav_fleet_stats
#include "mnav_plans_capi.h"      // mnav_upload_face_normals, mnav_fleet_plans, mnav_fleet_walk_plans
#include "mnav_dispatch_capi.h"   // mnav_fleet_costs, mnav_fleet_assign, mnav_dispatch_stats
#include "mnav_traffic_capi.h"    // mnav_fleet_traffic, mnav_traffic_download, mnav_traffic_stats, mnav_layer_traffic, mnav_map_traffic
#include "mnav_timed_capi.h"      // mnav_fleet_timed_traffic, mnav_timed_traffic_download, mnav_timed_traffic_stats, mnav_layer_timed_traffic, mnav_map_timed_traffic
#include "mnav_schedule_capi.h"   // mnav_fleet_schedule, mnav_schedule_stats

void mnav_cancel(mnav_ctx* ctx)
{
  if (!ctx) return;
  ctx->cancel.store(1, std::memory_order_relaxed);
  // thread-safe (MBF calls cancel() from the action-server thread), fire and forget: SDMA copy beside the running kernel
  if (ctx->d_cancel && ctx->h_one) (void)hipMemcpyAsync(ctx->d_cancel, ctx->h_one, 4, hipMemcpyHostToDevice, ctx->cancel_stream);
}

// The settled-vertex count of a paths-only tile-batch call is instrumentation (it only feeds mnav_stats.settled and
// mnav_algorithmic_bytes): it is taken from the resident distances on the first query after the call, not inside it.
static void settle_stats(mnav_ctx* ctx)
{
  if (!ctx->tb.count_pending) return;
  ctx->tb.count_pending = false;
  // only the arguments of a tile-batch call that succeeded and whose buffers are still allocated may be dereferenced
  if (!ctx->tb_args_valid || !ctx->res.dijkstra_family() || ctx->last_engine != 5 || !ctx->tb.built) return;
  const uint32_t m = ctx->res.live();
  if (!m || hipSetDevice(ctx->device) != hipSuccess) return;
  hipLaunchKernelGGL(k_tb_count, dim3(ctx->tb.ntiles ? ctx->tb.ntiles : 1, 16), dim3(kBlock), 0, ctx->stream, ctx->tb_args, ctx->tb.T, ctx->d_res);
  if (hipMemcpyAsync(ctx->h_res, ctx->d_res, sizeof(PlanResult) * m, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) return;
  finish_stats(ctx, m, false);
}

int mnav_get_stats(const mnav_ctx* ctx, mnav_stats* out)
{
  if (!ctx || !out) return -1;
  settle_stats(const_cast<mnav_ctx*>(ctx));
  *out = ctx->stats;
  return 0;
}

// What the last tile-batch call's finalize pass kept; the pairs are counted from the pass's maps here,
// on request, not inside the call.
int mnav_tb_finalize_stats(mnav_ctx* ctx, uint64_t* skipped_pairs, uint64_t* reset_pairs, uint32_t* filled_at_start)
{
  if (!ctx) return -1;
  TbState& S = ctx->tb;
  unsigned long long cnt[2] = { 0ull, 0ull };
  if (S.fin_stats && S.umap && S.fin_np && S.ntiles) {
    if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
    const uint32_t nblk = (S.fin_np + 63u) / 64u;
    HIPCHK(hipMemsetAsync(S.fin_cnt, 0, 16, ctx->stream));
    hipLaunchKernelGGL(k_tb_fin_count, dim3(std::min<uint32_t>(((size_t)S.ntiles * nblk + kBlock - 1) / kBlock, 1024u)), dim3(kBlock), 0, ctx->stream,
                       S.umap.get(), S.uskip.get(), S.ntiles, nblk, S.umap_stride, S.fin_cnt.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(cnt, S.fin_cnt, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  if (skipped_pairs) *skipped_pairs = cnt[1];
  if (reset_pairs) *reset_pairs = (S.fin_stats && S.fin_reset) ? (uint64_t)S.ntiles * S.fin_np - cnt[0] : 0u;
  if (filled_at_start) *filled_at_start = S.filled_at_start ? 1u : 0u;
  return 0;
}

int mnav_tb_engine_stats(const mnav_ctx* ctx, uint32_t* iterations, uint64_t* items, uint64_t* activations, uint64_t* sweeps, uint64_t* wakes)
{
  if (!ctx) return -1;
  const tb::Ctl& K = ctx->tb.last;
  if (iterations) *iterations = K.iters;
  if (items) *items = K.items;
  if (activations) *activations = K.acts;
  if (sweeps) *sweeps = K.sweeps;
  if (wakes) *wakes = K.wakes;
  return 0;
}

int mnav_get_timing(const mnav_ctx* ctx, mnav_stats* out)
{
  if (!ctx || !out) return -1;
  *out = ctx->stats;
  if (ctx->tb.count_pending) out->settled = 0;
  return 0;
}

int mnav_set_band_width(mnav_ctx* ctx, float delta)
{
  if (!ctx) return -1;
  ctx->delta_user = delta > 0.f ? delta : 0.f;
  return 0;
}

int mnav_set_dijkstra_engine(mnav_ctx* ctx, int engine)
{
  if (!ctx || engine < 0 || engine > 6 || engine == 2 || engine == 4) return -1;   // 2: one workgroup per plan, 4: one wave per plan (both retired)
  ctx->dij_engine = engine;
  ctx->opt.dijkstra_engine = (double)engine;
  return 0;
}

int mnav_set_option(mnav_ctx* ctx, const char* name, double value)
{
  if (!ctx || !name) return -1;
  double* f = ctx->opt.find(name);
  if (!f) { ctx->err = std::string("unknown option: ") + name; return -1; }
  if (!strcmp(name, "dijkstra_engine") && value == value) {           // the retired engines are refused like by mnav_set_dijkstra_engine
    const int e = (int)value;
    if (value != (double)e || e < 0 || e > 6 || e == 2 || e == 4) { ctx->err = "dijkstra_engine: 0, 1, 3 (auto), 5 or 6"; return -1; }
  }
  *f = value;                                                         // NaN: back to the built-in default
  apply_options(ctx);
  drop_graphs(ctx);                                                   // (captured launch sequences may hold what the option decides)
  return 0;
}

double mnav_get_option(const mnav_ctx* ctx, const char* name)
{
  if (!ctx || !name) return NAN;
  const double* f = const_cast<mnav_ctx*>(ctx)->opt.find(name);
  return f ? *f : NAN;
}

const void* mnav_device_output(const mnav_ctx* ctx, uint32_t slot, int what)
{
  if (!ctx) return nullptr;
  // the record decides (a stale slot of an earlier, larger batch, the dist of a paths-only call -- mnav_download_output what = 5
  // returns its popped potential --, an earlier call's vector map are never handed out); the slots may be gone with the mesh
  if (!ctx->res.available(slot, what) || ctx->res.slot(slot) >= ctx->slots.size()) return nullptr;
  const Slot& s = ctx->slots[ctx->res.slot(slot)];
  switch (what) {
    case 0: return s.dist;
    case 1: return s.pred;
    case 2: return s.dirn;
    case 3: return s.cutf;
    case 4: return s.vecmap;
    default: return nullptr;
  }
}

int mnav_set_resident_outputs(mnav_ctx* ctx, int on)
{
  if (!ctx) return -1;
  ctx->resident_vecmap = on != 0;
  return 0;
}

int mnav_download_output(mnav_ctx* ctx, uint32_t slot, int what, void* host_out)
{
  if (!ctx || !host_out) return -1;
  if (what == 5) {                                                   // popped potential (Dijkstra): exact wherever dist <= goal_dist, +inf elsewhere
    if (!ctx->res.dijkstra_family()) { ctx->err = "popped potential: the last call was not a Dijkstra plan"; return -1; }
    slot = ctx->res.slot_or_raw(slot);
    if (slot >= ctx->res.live()) { ctx->err = "output not resident"; return -1; }
    // The record keeps its live count through mnav_upload_mesh, the memory is gone with the old mesh: a paths-only tile-batch
    // call left its distances in the engine's buffers (no plan slot), every other call in slots[slot].dist
    const bool tb_paths_only = ctx->last_engine == 5 && ctx->res.paths_only();
    if (tb_paths_only ? !ctx->tb_args_valid : slot >= ctx->slots.size()) { ctx->err = "output not resident"; return -1; }
    if (hipSetDevice(ctx->device) != hipSuccess) return -1;
    DevBuf<float> tmp;
    HIPCHK(tmp.alloc(4 * (size_t)(ctx->V ? ctx->V : 1)));
    const uint32_t g = std::min<uint32_t>((ctx->V + kBlock - 1) / kBlock + 1, 4096);
    if (tb_paths_only) hipLaunchKernelGGL(k_tb_popped, dim3(g), dim3(kBlock), 0, ctx->stream, ctx->tb_args, slot, ctx->V, tmp);
    else hipLaunchKernelGGL(k_popped, dim3(g), dim3(kBlock), 0, ctx->stream, ctx->slots[slot].dist, ctx->res.robot_vertex(slot), ctx->res.offset(), ctx->V, tmp);
    const hipError_t e1 = hipMemcpyAsync(host_out, tmp, 4 * (size_t)ctx->V, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    tmp.reset();
    if (e1 != hipSuccess || e2 != hipSuccess) { ctx->err = "popped potential: copy failed"; return -1; }
    return 0;
  }
  const void* src = mnav_device_output(ctx, slot, what);
  if (!src) { ctx->err = "output not resident"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) return -1;
  const size_t bytes = (what == 4 ? 12 : 4) * (size_t)ctx->V;
  HIPCHK(hipMemcpyAsync(host_out, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

// MeshMap::directionAtPosition (mesh_map.cpp:625-650) on the resident vector map of plan `slot`: what the controller
// samples at the robot pose.  36 bytes cross PCIe instead of the 12 MB field.  A vertex counts as "has a vector" when
// its entry is not the all-zero vector the vector-map kernels write for vertices the wave did not set.
int mnav_vector_at(mnav_ctx* ctx, uint32_t slot, const uint32_t vs[3], const float bary[3], float out[3])
{
  if (!ctx || !vs || !bary || !out) return -1;
  for (int k = 0; k < 3; ++k) if (vs[k] >= ctx->V) { ctx->err = "vertex id out of range"; return -1; }
  float v[3][3];
  if (ctx->last_engine == 5 && ctx->res.paths_only() && ctx->tb_args_valid) {
    // paths-only batch of the tile-batch engine: no vector map was written -- the three entries are derived from the blocked distances
    const uint32_t p = ctx->res.slot_or_raw(slot);
    if (p >= ctx->res.live()) { ctx->err = "output not resident"; return -1; }
    if (hipSetDevice(ctx->device) != hipSuccess) return -1;
    if (!ctx->d_vec3) HIPCHK(ctx->d_vec3.alloc(64));
    hipLaunchKernelGGL(k_tb_vector3, dim3(3), dim3(kWave), 0, ctx->stream, ctx->tb_args, ctx->d_row_ptr, ctx->d_nbr, ctx->d_xyz, p,
                       make_uint3(vs[0], vs[1], vs[2]), ctx->d_vec3);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&v[0][0], ctx->d_vec3, 36, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  } else {
    const float* vm = static_cast<const float*>(mnav_device_output(ctx, slot, 4));
    if (!vm) { ctx->err = "vector map not resident"; return -1; }
    if (hipSetDevice(ctx->device) != hipSuccess) return -1;
    for (int k = 0; k < 3; ++k) HIPCHK(hipMemcpyAsync(v[k], vm + 3 * (size_t)vs[k], 12, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  float acc[3] = { 0.f, 0.f, 0.f };
  bool any = false;
  for (int k = 0; k < 3; ++k) {
    const bool has = !(v[k][0] == 0.f && v[k][1] == 0.f && v[k][2] == 0.f);
    if (!has) continue;
    any = true;
    for (int c = 0; c < 3; ++c) acc[c] += v[k][c] * bary[k];       // :636-638
  }
  if (!any || !(std::isfinite(acc[0]) && std::isfinite(acc[1]) && std::isfinite(acc[2]))) return 0;   // :639-646
  out[0] = acc[0]; out[1] = acc[1]; out[2] = acc[2];
  return 1;
}

// f3 of SURVEY.md section 8: the consumer of the CVP vector field on the device.  Plan i of the last mnav_plan_cvp(_batch)
// call is walked from its target (the robot) back to its seed (the goal) over the vector map resident in HBM; what
// crosses PCIe is the path, not the 12 B/vertex field.
int mnav_backtrack_cvp_batch(mnav_ctx* ctx, uint32_t n, const float* seed_pos, const uint32_t* seed_faces, const float* target_pos,
                             const uint32_t* target_faces, double step_width, int32_t inflation_layer, uint32_t cap, float* positions_out,
                             uint32_t* faces_out, uint32_t* n_out, int32_t* status_out)
{
  if (!ctx) return -1;
  ctx->err.clear();
  if (!n) return 0;
  if (!seed_pos || !seed_faces || !target_pos || !target_faces || !positions_out || !faces_out || !n_out || !status_out) { ctx->err = "null argument"; return -1; }
  if (cap < 2 || (uint64_t)cap * n > (1ull << 28)) { ctx->err = "path capacity out of range"; return -1; }
  if (!(step_width > 0.0)) { ctx->err = "step_width must be positive"; return -1; }   // a zero step never leaves the start
  if (ctx->res.kind() != Resident::kCvp) { ctx->err = "back-tracking: the last call was not a CVP plan"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  if (n != ctx->res.plans()) { ctx->err = "back-tracking: n differs from the last mnav_plan_cvp(_batch) call"; return -1; }
  std::vector<WalkJob> jobs(n);
  for (uint32_t i = 0; i < n; ++i) {
    const float* vm = static_cast<const float*>(mnav_device_output(ctx, i, 4));
    jobs[i].vecmap = nullptr;
    if (ctx->res.slot(i) == kNone) continue;                       // a plan rejected before it reached the device (INVALID_START / _GOAL): status 0, no entries
    if (!vm) { ctx->err = "vector map not resident (mnav_set_resident_outputs, or pass vecmap_out to the plan call)"; return -1; }
    if (seed_faces[i] >= ctx->F || target_faces[i] >= ctx->F) { ctx->err = "face id out of range"; return -1; }
    jobs[i].vecmap = vm; jobs[i].seed_face = seed_faces[i]; jobs[i].target_face = target_faces[i];
    for (int k = 0; k < 3; ++k) { jobs[i].seed[k] = seed_pos[3 * (size_t)i + k]; jobs[i].target[k] = target_pos[3 * (size_t)i + k]; }
  }
  WalkInflation L{};
  if (inflation_layer >= 0) {
    if ((size_t)inflation_layer >= ctx->layers.size() || !ctx->layers[inflation_layer].ready || !ctx->layers[inflation_layer].dist || !ctx->layers[inflation_layer].have_vec) {
      ctx->err = "back-tracking: not a resident inflation layer with a vector field"; return -1;
    }
    const mnav_ctx::Layer& Ly = ctx->layers[inflation_layer];
    L.distances = Ly.dist; L.vectors = Ly.vec; L.has_vector = Ly.vstate;
    L.inflation_radius = Ly.inflation_radius; L.inscribed_radius = Ly.inscribed_radius; L.inscribed_value = Ly.inscribed_value; L.lethal_value = Ly.lethal_value;
    L.repulsive_field = 1;
  }
  if (upload_walk_mesh(ctx)) return -1;
  const size_t need = (size_t)cap * n;
  if (need > ctx->walk_cap) {
    ctx->d_walk_pos.reset(); ctx->d_walk_face.reset(); ctx->walk_cap = 0;
    HIPCHK(ctx->d_walk_pos.alloc(12 * need)); HIPCHK(ctx->d_walk_face.alloc(4 * need));
    ctx->walk_cap = need;
  }
  if (n > ctx->walk_jobs_cap) {
    ctx->d_walk_jobs.reset(); ctx->d_walk_ctl.reset(); ctx->walk_jobs_cap = 0;
    HIPCHK(ctx->d_walk_jobs.alloc(sizeof(WalkJob) * (size_t)n)); HIPCHK(ctx->d_walk_ctl.alloc(8 * (size_t)n));
    ctx->walk_jobs_cap = n;
  }
  HIPCHK(hipMemcpyAsync(ctx->d_walk_jobs, jobs.data(), sizeof(WalkJob) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  WalkMesh M{ ctx->d_xyz, ctx->d_faces, ctx->d_vf_ptr, ctx->d_vf, ctx->V, ctx->F };
  hipLaunchKernelGGL(k_backtrack, dim3(n), dim3(64), 0, ctx->stream, M, L, ctx->d_walk_jobs, step_width, cap, ctx->d_walk_pos, ctx->d_walk_face, ctx->d_walk_ctl);
  HIPCHK(hipGetLastError());
  std::vector<int32_t> ctl(2 * (size_t)n);
  HIPCHK(hipMemcpyAsync(ctl.data(), ctx->d_walk_ctl, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (uint32_t i = 0; i < n; ++i) {                                  // the walked entries only: O(path) bytes per plan
    const uint32_t m = (uint32_t)ctl[2 * (size_t)i + 1];
    if (m) {
      HIPCHK(hipMemcpyAsync(positions_out + 3 * (size_t)cap * i, ctx->d_walk_pos + 3 * (size_t)cap * i, 12 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipMemcpyAsync(faces_out + (size_t)cap * i, ctx->d_walk_face + (size_t)cap * i, 4 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    }
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t m = (uint32_t)ctl[2 * (size_t)i + 1];
    float* pp = positions_out + 3 * (size_t)cap * i; uint32_t* pf = faces_out + (size_t)cap * i;
    for (uint32_t a = 0, b = m ? m - 1 : 0; a < b; ++a, --b) {        // the reference push_front()s: list order is seed first
      for (int k = 0; k < 3; ++k) std::swap(pp[3 * (size_t)a + k], pp[3 * (size_t)b + k]);
      std::swap(pf[a], pf[b]);
    }
    n_out[i] = m; status_out[i] = ctl[2 * (size_t)i];
  }
  return 0;
}

int mnav_backtrack_cvp(mnav_ctx* ctx, const float seed_pos[3], uint32_t seed_face, const float target_pos[3], uint32_t target_face, double step_width,
                       int32_t inflation_layer, uint32_t cap, float* positions_out, uint32_t* faces_out, uint32_t* n_out)
{
  int32_t status = 0;
  const int rc = mnav_backtrack_cvp_batch(ctx, 1, seed_pos, &seed_face, target_pos, &target_face, step_width, inflation_layer, cap, positions_out, faces_out, n_out, &status);
  return rc < 0 ? rc : status;
}

uint64_t mnav_algorithmic_bytes(const mnav_ctx* ctx)
{
  if (!ctx) return 0;
  settle_stats(const_cast<mnav_ctx*>(ctx));
  return ctx->algo_bytes;
}

int mnav_last_engine(const mnav_ctx* ctx)
{
  if (!ctx || !ctx->res.dijkstra_family() || ctx->res.live() == 0) return -1;
  if (ctx->mesh_since_outputs) return -1;                             // a new mesh since the call: its fields are gone, the record's live count is not
  if (ctx->rp.each_engines) return ctx->rp.each_engines;
  return ctx->last_engine + ((ctx->last_engine == 5 && ctx->tb.kernel == 1) ? 16 : 0);
}

#ifdef MNAV_TILE_TIMING
int mnav_debug_tile_timing(unsigned long long* out, unsigned int cap)
{
  unsigned int n = 0;
  (void)hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_tile_timing_n), sizeof(n));
  if (n > 4096) n = 4096;
  if (n > cap) n = cap;
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tile_timing), sizeof(unsigned long long) * 8 * n);
  unsigned int z = 0;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_tile_timing_n), &z, sizeof(z));
  return (int)n;
}
#endif

}  // extern "C"

#ifdef MNAV_WIDE_TIMING
extern "C" int mnav_debug_wide_timing(unsigned long long* out)
{
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wide_timing), sizeof(unsigned long long) * 12) != hipSuccess) return -1;
  unsigned long long z[12] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
  return hipMemcpyToSymbol(HIP_SYMBOL(g_wide_timing), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif
