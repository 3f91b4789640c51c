/*
 * mnav.h -- C ABI of the MI355X-native wavefront planner (libmnav.so).
 *
 * The reference has no C ABI: its boundary is the C++ pure-virtual plugin class
 * mbf_mesh_core::MeshPlanner (mbf_mesh_core/include/mbf_mesh_core/mesh_planner.h:50-92)
 * loaded through pluginlib.  This header is what a MeshPlanner implementation binds
 * instead of running the priority-queue loops itself; INTEGRATION.md shows the
 * adapter (mesh_navigation_amd/csrc/adapter/) that keeps makePlan / cancel /
 * initialize unchanged on top of it.
 *
 * Conventions: plain pointers and sizes only; the caller owns every buffer it
 * passes; the context owns all device memory; one plan call in flight per
 * context (the reference reuses potential_/predecessors_ members the same way,
 * dijkstra_mesh_planner.h:189-197).  Vertex / face / edge ids are the
 * reference's handles' idx() values.  All plan functions return the MBF GetPath
 * result codes of dijkstra_mesh_planner.h:72-85.  The library never computes on
 * the CPU: without a usable GPU mnav_create() fails (returns NULL).
 */
#ifndef MNAV_H
#define MNAV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MNAV_SUCCESS 0u         /* mbf_msgs GetPath::Result::SUCCESS        */
#define MNAV_CANCELED 51u       /* ...::CANCELED                            */
#define MNAV_INVALID_START 52u  /* ...::INVALID_START                       */
#define MNAV_INVALID_GOAL 53u   /* ...::INVALID_GOAL                        */
#define MNAV_NO_PATH_FOUND 54u  /* ...::NO_PATH_FOUND                       */
#define MNAV_INTERNAL_ERROR 60u /* ...::INTERNAL_ERROR (device/runtime failure) */
#define MNAV_NONE 0xFFFFFFFFu

typedef struct mnav_ctx mnav_ctx;

/* Per-call statistics (the phases the reference logs, dijkstra_mesh_planner.cpp:391-394,
 * cvp_mesh_planner.cpp:956-960).  Times are HIP-event milliseconds on the context stream. */
typedef struct mnav_stats {
  uint32_t steps;          /* wavefront step-kernel launches that did work       */
  uint32_t launches;       /* step launches enqueued (incl. overshoot no-ops)    */
  uint32_t bands;          /* distance bands completed                           */
  uint32_t armed;          /* goal_dist was armed                                */
  float goal_dist;         /* armed value or +inf                                */
  uint32_t n_plans;        /* plans in the call (batch size)                     */
  uint64_t evals;          /* vertex evaluations (all plans)                     */
  uint64_t settled;        /* vertices with a finite potential (all plans)       */
  float ms_init;           /* state initialisation                               */
  float ms_propagation;    /* wavefront propagation (all step launches)          */
  float ms_vector_map;     /* computeVectorMap                                   */
  float ms_path;           /* predecessor walk                                   */
  float ms_download;       /* device -> host copies of requested outputs         */
  float ms_total;          /* whole call                                         */
  float ms_step_kernels;   /* sum over graph replays of the event-bracketed step/round launches
                              (excludes the host polls between replays)          */
  uint32_t band_shrinks;   /* bands cut down because they did not converge (all plans)   */
  uint32_t band_cuts;      /* bands restarted under a lower bound after kCutAfter steps     */
} mnav_stats;

/* -- life cycle -------------------------------------------------------------------------- */
/* Replaces: plugin construction + MeshPlanner::initialize(name, mesh_map, node),
 * mesh_planner.h:88 (dijkstra_mesh_planner.cpp:142-169, cvp_mesh_planner.cpp:148-186). */
mnav_ctx* mnav_create(int device);
void mnav_destroy(mnav_ctx* ctx);
/* Text of the last failure on this context ("" if none); valid until the next call. */
const char* mnav_last_error(const mnav_ctx* ctx);

/* Upload the half-edge mesh once (MeshMap::mesh(), mesh_map.h:276-279) as flat arrays:
 * xyz V*3, face_vtx F*3 (reference face order), edge_vtx E*2 (reference edge ids),
 * vertex_normals V*3 (MeshMap::vertexNormals(), mesh_map.h:326-337; may be NULL if only the
 * Dijkstra planner is used: mnav_plan_cvp needs them for its vector map).  Returns 0 on success,
 * <0 on error. */
int mnav_upload_mesh(mnav_ctx* ctx, uint32_t V, uint32_t F, uint32_t E, const float* xyz,
                     const uint32_t* face_vtx, const uint32_t* edge_vtx,
                     const float* vertex_normals);

/* Optional, BEFORE mnav_upload_mesh: the rows of lvr2::PMPMesh::getFacesOfVertex (half-edge circulator
 * order) as CSR, vf_ptr V+1, vf 3F.  CVPMeshPlanner applies the faces of a popped vertex in that order
 * (cvp_mesh_planner.cpp:775-778) and its update is not a pure minimum on cost-inflated triangles, so the
 * order is part of the result.  Without this call (or with NULL rows) the library derives the order itself
 * by replaying pmp::SurfaceMesh::add_face over face_vtx in index order, which is how the reference builds
 * its mesh from the map file (mesh_map.cpp:273).  Returns 0. */
int mnav_set_face_circulation(mnav_ctx* ctx, uint32_t V, uint32_t F, const uint32_t* vf_ptr,
                              const uint32_t* vf);

/* Upload the inputs the planners re-read on every plan (dijkstra_mesh_planner.cpp:214,
 * cvp_mesh_planner.cpp:245): vertex_costs V (MeshMap::vertexCosts(), mesh_map.h:292-295),
 * edge_weights E (MeshMap::edgeWeights(), mesh_map.h:342-345), invalid V bytes
 * (MeshMap::invalid, mesh_map.h:447; NULL = none). */
int mnav_upload_costs(mnav_ctx* ctx, const float* vertex_costs, const float* edge_weights,
                      const uint8_t* invalid);

/* Device version of MeshMap::computeEdgeWeights (mesh_map/src/mesh_map.cpp:517-561): uploads
 * vertex_costs V and edge_distances E and derives the edge weights on the GPU with the
 * reference's mixed float/double arithmetic.  edge_weights_out (E, may be NULL) receives them. */
int mnav_compute_edge_weights(mnav_ctx* ctx, const float* vertex_costs, const float* edge_distances,
                              double edge_cost_factor, const uint8_t* invalid,
                              float* edge_weights_out);

/* Device version of the combination layers that produce the planners' vertex costs
 * (mesh_layers/src/combination_layer.cpp:44-85 MaxCombinationLayer, :185-248 AvgCombinationLayer; the
 * default layer copied by MeshMap::copyVertexCostsFromDefaultLayer, mesh_map.cpp:495-515), followed by
 * the edge weights of mnav_compute_edge_weights: mode 0 = max, 1 = weighted sum (weights n_layers,
 * AbstractLayer::combinationWeight()); layer_costs = n_layers dense V-sized arrays (missing entries
 * already replaced by the layer's default value), combined in the given order starting from 0.
 * The result becomes the context's vertex costs / edge weights; vertex_costs_out V and
 * edge_weights_out E (either may be NULL) receive copies. */
int mnav_combine_costs(mnav_ctx* ctx, int mode, uint32_t n_layers, const float* const* layer_costs,
                       const float* weights, const float* edge_distances, double edge_cost_factor,
                       const uint8_t* invalid, float* vertex_costs_out, float* edge_weights_out);

/* -- planning ---------------------------------------------------------------------------- */
/* Replaces DijkstraMeshPlanner::dijkstra (7-arg) + computeVectorMap,
 * dijkstra_mesh_planner.cpp:217-398, :189-209.  seed_vertex = wave seed (navigation goal),
 * target_vertex = robot vertex (both already resolved by MeshMap::getNearestVertexHandle,
 * :235-236).  Outputs (any may be NULL): dist_out V (potential_), pred_out V
 * (predecessors_), vecmap_out V*3 (vector_map_, zero rows where the reference has no entry),
 * path_out/path_len: the vertex path in dijkstra()'s list order (seed first ... pred[target]),
 * at most path_cap entries are written, *path_len is the full length.
 * goal_dist_offset: any double like the reference's parameter (default 0.3).  A negative value stops the expansion at the
 * robot vertex (only vertices popped before it are sources, :293-300) and is reproduced exactly; NaN is refused.  The CVP
 * and sharded entry points below take negative offsets too (CVP: every pop up to and including the arming one expands,
 * cvp_mesh_planner.cpp:754 before :765-769). */
uint32_t mnav_plan_dijkstra(mnav_ctx* ctx, uint32_t seed_vertex, uint32_t target_vertex,
                            double goal_dist_offset, double cost_limit, float* dist_out,
                            uint32_t* pred_out, uint32_t* path_out, uint32_t path_cap,
                            uint32_t* path_len, float* vecmap_out);

/* Replaces CVPMeshPlanner::waveFrontPropagation up to and including computeVectorMap,
 * cvp_mesh_planner.cpp:651-918, :204-239 (the vector-field back-tracking :920-951 stays on
 * the host, see the adapter).  seed_pos = exact wave seed position (navigation goal),
 * seed_face / target_face = containing faces (MeshMap::getContainingFace, :673-674).
 * Outputs (any may be NULL): dist_out V, pred_out V, direction_out V (direction_),
 * cutface_out V (cutting_faces_, MNAV_NONE = no entry), vecmap_out V*3.  Entries of
 * direction/cutface/vecmap for vertices the wave did not update are 0 / MNAV_NONE / 0
 * (the reference leaves stale values of earlier plans there, cvp_mesh_planner.cpp:179). */
uint32_t mnav_plan_cvp(mnav_ctx* ctx, const float seed_pos[3], uint32_t seed_face,
                       uint32_t target_face, double goal_dist_offset, double cost_limit,
                       float* dist_out, uint32_t* pred_out, float* direction_out,
                       uint32_t* cutface_out, float* vecmap_out);

/* n independent Dijkstra plans on the same mesh in one sweep (BASELINE config 5: concurrent
 * goals).  seeds/targets: n each.  codes_out n.  dist_out/pred_out: n*V or NULL.
 * path_out: n*path_cap or NULL, path_len n.  * A call that asks for nothing V-sized (dist_out, pred_out, vecmap_out all NULL, resident outputs off) only derives the
 * predecessors along the returned path (no finalize pass over the touched tiles): mnav_device_output(slot, pred) is
 * NULL afterwards and the resident potential is final up to goal_dist only.  MNAV_LAZY_PATHS=0 restores the full pass.
 */
uint32_t mnav_plan_dijkstra_batch(mnav_ctx* ctx, uint32_t n, const uint32_t* seeds,
                                  const uint32_t* targets, double goal_dist_offset,
                                  double cost_limit, uint32_t* codes_out, float* dist_out,
                                  uint32_t* pred_out, uint32_t* path_out, uint32_t path_cap,
                                  uint32_t* path_len);

/* n independent CVP plans on the same mesh in one sweep.  seed_pos n*3, seed_faces / target_faces n,
 * codes_out n; dist_out / pred_out n*V, vecmap_out n*V*3 or NULL. */
uint32_t mnav_plan_cvp_batch(mnav_ctx* ctx, uint32_t n, const float* seed_pos, const uint32_t* seed_faces,
                             const uint32_t* target_faces, double goal_dist_offset, double cost_limit,
                             uint32_t* codes_out, float* dist_out, uint32_t* pred_out, float* vecmap_out);

/* Incremental cost change: MeshMap::layerChanged (mesh_map.cpp:454-493) + updateEdgeWeights(changed) (:563-618) on
 * the device.  The n vertices get their new costs; if the resident weights were computed here with a non-zero
 * edge_cost_factor (mnav_compute_edge_weights / mnav_combine_costs) the edges around them are re-weighted with the
 * same mixed float/double expression (:606-610), otherwise only the vertex costs change ("edge_cost_factor is 0,
 * skipping edge cost update", :568-572).  Nothing but the n ids and values crosses PCIe.  Returns 0 / <0. */
int mnav_update_costs(mnav_ctx* ctx, uint32_t n, const uint32_t* vertex_ids, const float* values);
/* The caller's own incremental edge weights (MeshMap::updateEdgeWeights, mesh_map.cpp:563-618, already run on the host by
 * MeshMap::layerChanged :454-493): `values[i]` replaces the weight of edge `edge_ids[i]`.  Together with mnav_update_costs on
 * weights that were uploaded (mnav_upload_costs: then mnav_update_costs only touches the vertex costs) a cost change of the
 * map costs O(changed) instead of a pass over all vertices and edges. */
int mnav_update_edge_weights(mnav_ctx* ctx, uint32_t n, const uint32_t* edge_ids, const float* values);
/* Copies of the resident vertex costs (V) and edge weights (E); either pointer may be NULL. */
int mnav_download_costs(mnav_ctx* ctx, float* vertex_costs_out, float* edge_weights_out);

/* -- cost layers on the device (mesh_layers) ------------------------------------------------------
 * The reference's layer plugins compute per-vertex costs on the CPU (AbstractLayer::computeLayer) and MeshMap
 * combines them.  These entry points keep that stack in HBM: layer `k` (0..63) is a resident cost array + lethal set.
 *   mnav_layer_upload      a layer computed elsewhere (a costs file, a layer plugin without a device version ...): costs
 *                          V floats, lethal V bytes or NULL
 *   mnav_layer_obstacle    ObstacleLayer::processPointCloud (obstacle_layer.cpp:216-290) from a point cloud: see below
 *   mnav_layer_steepness   SteepnessLayer::computeLayer (steepness_layer.cpp:157-166) from the resident vertex normals:
 *                          cost = acos(n.z) in float, lethal when > threshold (:82-93)
 *   mnav_layer_inflation   InflationLayer::computeLayer (inflation_layer.cpp:96-178): the lethal set of `input_layer`
 *                          is the source of waveCostInflation (:341-491), a multi-source ordered fast-marching wave over
 *                          the edge distances, run here on the same ordered-wave engine as the CVP planner (replay of the
 *                          face updates in the reference's pop order, float32 Sethian update :181-234, re-queue rule
 *                          :311, invalid vertices never fixed :417); then riskiness = fading(distance) (:315-339).
 *                          `invalid` = the map's non-manifold flags (V bytes) or NULL.  Distances are bit-identical to
 *                          the reference's; a converged state that fails the verification sweep returns <0 instead of a
 *                          result; it works in the first plan slot, so the resident outputs of the last plan are gone
 *                          afterwards (mnav_download_output fails until the next plan).  The layer's repulsive vector field (vector_map_, :277-309: an order-dependent
 *                          accumulation over the lethal contours, then assignments in pop order) is computed as well
 *                          (mnav_layer_download_vectors), under the (value, id) heap-tie convention of the library.
 *   mnav_layer_download    copies of a layer's costs / lethal flags / wave distances (NULL to skip; distances only for an
 *                          inflation layer, +inf where the wave never arrived)
 *   mnav_combine_layers    CombinationLayer (mode 0 = max :44-85, 1 = weighted sum :185-248) over resident layers, then
 *                          MeshMap::computeEdgeWeights (mesh_map.cpp:495-561): the resident vertex costs and edge weights
 *                          the planners read are replaced; edge distances are computed on the device if none are resident
 * All return 0 / <0 (mnav_last_error). */
int mnav_layer_upload(mnav_ctx* ctx, uint32_t layer, const float* costs, const uint8_t* lethal);
int mnav_layer_steepness(mnav_ctx* ctx, uint32_t layer, double threshold);
int mnav_layer_inflation(mnav_ctx* ctx, uint32_t layer, uint32_t input_layer, double inflation_radius, double inscribed_radius,
                         double inscribed_value, double lethal_value, double cost_scaling_factor, const uint8_t* invalid);
int mnav_layer_download(mnav_ctx* ctx, uint32_t layer, float* costs_out, uint8_t* lethal_out, float* distances_out);
/* vector_map_ of an inflation layer: V*3 floats and V flags (1 = the reference's map holds an entry); NULL to skip. */
int mnav_layer_download_vectors(mnav_ctx* ctx, uint32_t layer, float* vectors_out, uint8_t* has_vector_out);
int mnav_combine_layers(mnav_ctx* ctx, int mode, uint32_t n_layers, const uint32_t* layers, const float* weights,
                        double edge_cost_factor, const uint8_t* invalid);
/* CombinationLayer::onInputChanged (combination_layer.cpp:87-147, :250-302) + MeshMap::layerChanged (mesh_map.cpp:454-493)
 * + updateEdgeWeights(changed) (:563-618): after a layer changed on n vertices (re-uploaded or recomputed on the device)
 * only those vertices are recombined and only the edges around them re-weighted.  Same mode / layers / weights as the full
 * mnav_combine_layers that came before. */
int mnav_combine_layers_update(mnav_ctx* ctx, int mode, uint32_t n_layers, const uint32_t* layers, const float* weights, uint32_t n,
                               const uint32_t* vertex_ids);
/* Counters of the last inflation wave: band steps, bands, vertex evaluations, device milliseconds (whole call), fixing
 * verification sweeps that were needed, device milliseconds of the wave alone.  Any pointer may be NULL. */
int mnav_layer_stats(const mnav_ctx* ctx, uint32_t* steps, uint32_t* bands, uint64_t* evals, float* ms, uint32_t* verify_sweeps,
                     float* ms_wave);
/* ObstacleLayer::processPointCloud (obstacle_layer.cpp:216-290) on the device: n_points points of point_step bytes each
 * (x, y, z float32 at offsets 0, 4, 8, as PointCloud2 lays them out) are copied in, and layer `layer` becomes the
 * obstacle layer of that cloud.  Per point p (sensor frame):
 *   kept iff (double)sqrtf((x*x + y*y) + z*z) <= max_obstacle_dist (NaN points are dropped);
 *   origin o = R p + t, sensor_to_map a row-major 3x4 float matrix (NULL = identity), each row ((m0 x + m1 y) + m2 z) + m3;
 *   ray along down_axis (3 floats, already in the map frame, used as given: not re-normalised; must be finite, non-zero);
 *   cast with the watertight ray/triangle test of Woop, Benthin & Wald 2013 (mesh_navigation_amd/csrc/mnav_ray.h),
 *   two-sided, t >= 0, closest hit, equal t to the smallest face id, degenerate faces (det == 0) never hit, over a linear
 *   BVH of the resident faces that is built on the first call after mnav_upload_mesh;
 *   a hit with (double)t <= robot_height makes the face's three vertices lethal (both limits: +inf = no limit).
 * The layer's costs become +inf on lethal vertices and 0 elsewhere; its lethal flags become the new set.  changed_out
 * (capacity V, or NULL) receives the ascending ids whose lethal flag differs from the layer's flags before the call (a slot
 * that held no layer counts as empty): the `changed` set of the reference's notifyChange (:265-278), ready for
 * mnav_layer_inflation (with this layer as input) and mnav_combine_layers_update.  An empty cloud clears the layer.
 * Departures from the reference: the reference's raycaster is Embree or lvr2's BVH (mesh_map.cpp:312-324), neither of which
 * pins edge / tie behaviour; Eigen's summation order of R p is not pinned; a ray whose origin is not finite hits nothing.
 * Returns 0 / <0 (mnav_last_error). */
int mnav_layer_obstacle(mnav_ctx* ctx, uint32_t layer, uint32_t n_points, const void* points, uint32_t point_step,
                        const float* sensor_to_map, const float* down_axis, double robot_height, double max_obstacle_dist,
                        uint32_t* changed_out, uint32_t* n_changed, uint32_t* n_lethal);
/* Counters of the last mnav_layer_obstacle: rays kept by the distance filter, rays that hit a face, rays that made a face
 * lethal, device milliseconds of the last BVH build, of the ray cast kernel and of the whole call.  Any pointer may be NULL. */
int mnav_obstacle_stats(const mnav_ctx* ctx, uint32_t* rays_kept, uint32_t* hits, uint32_t* lethal_rays, float* ms_bvh_build,
                        float* ms_cast, float* ms_total);
/* The local-neighbourhood layers on the device: HeightDiffLayer (height_diff_layer.cpp:103-110), RoughnessLayer
 * (roughness_layer.cpp:144) and RidgeLayer (ridge_layer.cpp:155-184).  Per vertex v:
 *   N(v)       the vertices reachable from v over mesh edges along a path whose every vertex u has (double)d2(u) < radius *
 *              radius (radius * radius in double, strict); d2 = (dx*dx + dy*dy) + dz*dz in float, d = p_u - p_v, no
 *              contraction (lvr2 BaseVector::squaredDistanceFrom).  v is always a member; a vertex without edges has
 *              N(v) = {v}.  N(v) is a set: each member counts once, whatever order the visit takes.
 *   height     max z - min z over N(v), world z, subtracted in float (no normals needed)
 *   roughness  the mean over N(v) of acos(clamp(dot(n_v, n_u), -1, 1)), dot = (ax*bx + ay*by) + az*bz in float, acos = the
 *              host libm's acosf (the restatement used by mnav_layer_steepness)
 *   ridge      the mean over N(v) of sqrtf(|(p_u + n_u) - (p_v + n_v)|^2), additions in float, squared length as d2
 *   mean       each float term t becomes llrint((double)t * 2^32) (half to even); the int64 sum S gives
 *              (float)(((double)S * 2^-32) / (double)|N(v)|): order-free, so the result is deterministic bit for bit
 * The layer's costs become the values, its lethal flags (double)value > threshold (computeLethals).  Roughness and ridge
 * read the resident vertex normals and fail without them.  radius must be finite and >= 0; a ridge call needs
 * V * (2 * radius + 2) < 2^31 (the int64 sum cannot overflow).  Layer slots as for mnav_layer_steepness.  Departures from
 * lvr2 (whose sources the spec could not be checked against: INTEGRATION.md): a vertex met twice by lvr2's DFS would count
 * twice there; the mean is summed in fixed point, not in float in DFS order; the clamp of the dot product.
 * Reference defaults: height_diff threshold 0.185, radius 0.3; roughness and ridge threshold 0.3, radius 0.3.
 * Returns 0 / <0 (mnav_last_error); on error the layer is left untouched. */
int mnav_layer_height_diff(mnav_ctx* ctx, uint32_t layer, double radius, double threshold);
int mnav_layer_roughness(mnav_ctx* ctx, uint32_t layer, double radius, double threshold);
int mnav_layer_ridge(mnav_ctx* ctx, uint32_t layer, double radius, double threshold);
/* last call: centres, sum of |N(v)|, largest |N(v)|, centres that left the LDS path, device ms; NULL to skip */
int mnav_neighbourhood_stats(const mnav_ctx* ctx, uint32_t* centres, uint64_t* visits, uint32_t* max_size,
                             uint32_t* spilled, float* ms);
/* BorderLayer (border_layer.cpp:104-110, computeLethals :66-80) on the device.  v is a border vertex iff at least one edge
 * of its CSR row (the edges listed at upload that have v as an end) has fewer than two incident faces among the uploaded
 * faces: lvr2's calcBorderCosts as the library understands it.  A vertex without edges is not a border
 * vertex.  cost = (float)border_cost on border vertices, 0.0f elsewhere; lethal iff (double)cost > threshold (lethal
 * vertices keep border_cost, not +inf).  Reference defaults: threshold 0.5, border_cost 1.0 (border_layer.h:132-133).
 * border_cost must be finite and threshold not NaN.
 *
 * ClearanceLayer (clearance_layer.cpp:122-164, computeLethalsAndCosts :67-99) on the device.  The clearance c(v) of a
 * vertex is the closest hit of one ray that starts at p_v exactly (no epsilon offset) and runs along the resident normal
 * n_v as given (not re-normalised), cast with the obstacle layer's watertight test (mesh_navigation_amd/csrc/mnav_ray.h:
 * two-sided, t >= 0, closest hit, equal t to the smallest face id, degenerate faces never hit) over every face that does
 * NOT have v as a corner (compared by vertex id, not by position); c(v) = t of that hit, +inf without one.  A vertex whose
 * normal is not finite or is the zero vector gets +inf and casts no ray.  A hit at t = 0 on a face without v (coincident
 * sheets) counts: c = 0.  Costs, evaluated in double and stored as float:
 *   c < robot_height                       cost 1.0, lethal
 *   c < robot_height + height_inflation    cost (cos(((c - robot_height) / height_inflation) * pi) + 1.0) / 2.0
 *   otherwise                              cost 0
 * Reference defaults: robot_height 0.5, height_inflation 0.3 (clearance_layer.h:135-136); both must be finite and >= 0.
 * The clearance array is cached on the context (the reference's clearance_): the first call after mnav_upload_mesh builds
 * the obstacle layer's BVH if no mnav_layer_obstacle has built it yet, then casts; later calls only re-run the cost pass
 * (reconfigureCallback, :171-194).  mnav_upload_mesh drops the cache, as it drops the BVH.  The call needs resident
 * vertex normals.  A BVH built by this call is the one mnav_layer_obstacle then uses, and mnav_obstacle_stats'
 * ms_bvh_build reports it: the only effect on another entry point.
 *
 * Both: changed_out (capacity V, or NULL) receives the ascending ids whose lethal flag or cost bits differ from what the
 * slot held before the call (a slot that held no layer: every vertex), ready for mnav_combine_layers_update and
 * mnav_layer_inflation; n_changed / n_lethal (may be NULL) the sizes of the change list and of the new lethal set.  Layer
 * slots as for mnav_layer_steepness.  Returns 0 / <0 (mnav_last_error); on an argument error (no mesh, a bad parameter,
 * no normals) or a BVH traversal-stack overflow (which also drops the cache) the slot is left untouched. */
int mnav_layer_border(mnav_ctx* ctx, uint32_t layer, double border_cost, double threshold, uint32_t* changed_out, uint32_t* n_changed,
                      uint32_t* n_lethal);
int mnav_layer_clearance(mnav_ctx* ctx, uint32_t layer, double robot_height, double height_inflation, uint32_t* changed_out,
                         uint32_t* n_changed, uint32_t* n_lethal);
/* The cached clearance (V floats, +inf where nothing was hit); <0 when no clearance is cached. */
int mnav_clearance_download(const mnav_ctx* ctx, float* clearance_out);
/* The last mnav_layer_clearance: cast = 1 if it cast the rays, 0 if it reused the cache; rays cast and rays that hit by
 * that call (0 when reused); device milliseconds of the BVH build it ran (0 if none), of the cast kernel (0 if reused) and
 * of the whole call.  Any pointer may be NULL. */
int mnav_clearance_stats(const mnav_ctx* ctx, uint32_t* cast, uint32_t* rays, uint32_t* hits, float* ms_bvh_build, float* ms_cast,
                         float* ms_total);

/* -- the resident layer graph ------------------------------------------------------------------------
 * mesh_map::LayerManager (layer_manager.cpp:153-263) + MeshMap::layerChanged (mesh_map.cpp:454-493) on the device: the
 * layer stack is declared once; after that one call per event brings every dependent layer, the resident vertex costs and
 * the edge weights to the state the reference's notification chain (notifyChange -> LayerManager::layer_changed ->
 * MeshMap::layerChanged -> updateEdgeWeights(changed), plus onInputChanged of every dependent layer) would leave.  Between
 * the stages only counters cross PCIe; the change lists stay on the device.
 *
 * A node is a layer slot.  An INPUT node is a slot the caller fills with any writer (mnav_layer_upload, _steepness,
 * _height_diff, _roughness, _ridge, _border, _clearance, _obstacle).  Derived nodes are owned by the graph:
 *   INFLATION     mnav_layer_inflation of its one input with the node's five parameters
 *   COMBINE_MAX   cost = max over the inputs, from 0.0f, in input order (combination_layer.cpp:44-85)
 *   COMBINE_AVG   cost = sum of weights[k] * input k, from 0.0f, in input order, float multiply then float add (:185-248)
 *                 both: lethal flag = OR of the inputs' flags (:73-79, :122-139); a NaN cost never replaces the running max
 * so a combination is a layer like any other: it can feed an inflation or another combination. */
enum { MNAV_NODE_INPUT = 0, MNAV_NODE_INFLATION = 1, MNAV_NODE_COMBINE_MAX = 2, MNAV_NODE_COMBINE_AVG = 3 };
typedef struct {
  uint32_t layer;            /* slot 0..63 */
  uint32_t kind;
  uint32_t n_inputs;         /* INPUT: 0; INFLATION: exactly 1; COMBINE_*: 1..8 */
  uint32_t inputs[8];        /* slots of other nodes */
  float    weights[8];       /* COMBINE_AVG: combinationWeight of each input, in input order */
  double   inflation_radius, inscribed_radius, inscribed_value, lethal_value, cost_scaling_factor;  /* INFLATION */
} mnav_map_node;
/* Declares the graph (after mnav_upload_mesh; the next mnav_upload_mesh drops it).  default_layer is the node whose costs
 * become the vertex costs the planners read (any kind); edge_cost_factor and invalid (V bytes or NULL: the map's
 * non-manifold flags, read by the inflation waves and the planners) are those of mnav_combine_layers.  Returns <0 with a
 * mnav_last_error text, and leaves a previous configuration in place and usable, for: a slot out of range or listed
 * twice, an input that is not a node, a wrong n_inputs for the kind, a cycle, a default layer that is not a node.  The
 * order of evaluation is a dependency order (inputs before users; among ready nodes, the order of `nodes`). */
int mnav_map_configure(mnav_ctx* ctx, uint32_t n_nodes, const mnav_map_node* nodes, uint32_t default_layer, double edge_cost_factor,
                       const uint8_t* invalid);
/* The layer part of MeshMap::readMap (mesh_map.cpp:427-448): every INPUT slot must be resident; the derived nodes are
 * computed in order, the default layer is copied into the resident vertex costs (copyVertexCostsFromDefaultLayer) and the
 * full edge-weight pass runs (as mnav_combine_layers).  An inflation node works in the first plan slot, as
 * mnav_layer_inflation does: the resident outputs of the last plan are gone afterwards.  That holds for the three update
 * calls below whenever they re-run a wave. */
int mnav_map_compute(mnav_ctx* ctx);
/* The run-time chain, after a successful mnav_map_compute.  Each call names an INPUT node (a derived node is refused):
 *   mnav_map_update_layer   vertex_ids[i] takes costs[i] and, unless lethal is NULL, the flag lethal[i] (the harness's
 *                           ArrayLayer::update: duplicates allowed, of equal ids the last one counts); the layer's change
 *                           list is the given ids.  An id >= V is an error raised before anything is written.
 *   mnav_map_layer_changed  the caller rewrote the slot through one of the writers above and reports the vertices that
 *                           changed (e.g. the changed_out of mnav_layer_border); which lethal flags flipped is not known
 *                           here, so an inflation node on this input re-runs its wave whenever n > 0
 *   mnav_map_obstacle       mnav_layer_obstacle on the slot (same arguments from n_points to max_obstacle_dist); its change
 *                           list never leaves the device
 *   mnav_map_traffic        (declared with the fleet traffic calls below) mnav_layer_traffic on the slot, in the same way
 * Then every dependent node is visited in dependency order with the union of the change lists of its inputs that changed
 * in this call.  A combination recombines those vertices (cost and flag); its own list is the subset whose cost bits or
 * flag now differ.  An inflation node whose input had no lethal flag flipped on the list is left alone and emits nothing
 * (waveCostInflation is a function of the lethal set only); otherwise the wave is re-run whole, as the reference does
 * (inflation_layer.cpp:143), and its list is the vertices whose cost bits or flag differ from before.  Finally, for the
 * default layer's list D: the resident vertex costs take the layer's values on D, the edges around D are re-weighted if
 * edge_cost_factor != 0 (mesh_map.cpp:568-572), the host's cost mirror takes the |D| (id, value) pairs -- the only id-sized
 * download of the call -- and the cost-limit folded planner tables are rebuilt by the next plan.  changed_out (capacity V,
 * or NULL) receives D ascending, n_changed (or NULL) its length.
 * Departure from the reference: it forwards larger sets (a combination its whole incoming set, an inflation every vertex
 * either wave reached); recombining and re-weighting are idempotent, so every layer's costs and flags, the inflation
 * distances and vector field, the vertex costs and the edge weights are the same bit for bit, but the list reported here
 * is the tighter one: the vertices whose default-layer cost bits (or flag) changed.
 * A wave that fails its verification sweep, or any other failure after the first write, returns <0 and marks the graph
 * stale: the update calls then fail until a mnav_map_compute succeeds.  Writers used on an INPUT slot without a following
 * mnav_map_layer_changed, and mnav_upload_costs / mnav_combine_* on a context with a graph, leave the graph's state behind;
 * mnav_map_compute brings it back. */
int mnav_map_layer_changed(mnav_ctx* ctx, uint32_t layer, uint32_t n, const uint32_t* vertex_ids, uint32_t* changed_out, uint32_t* n_changed);
int mnav_map_update_layer(mnav_ctx* ctx, uint32_t layer, uint32_t n, const uint32_t* vertex_ids, const float* costs, const uint8_t* lethal,
                          uint32_t* changed_out, uint32_t* n_changed);
int mnav_map_obstacle(mnav_ctx* ctx, uint32_t layer, uint32_t n_points, const void* points, uint32_t point_step, const float* sensor_to_map,
                      const float* down_axis, double robot_height, double max_obstacle_dist, uint32_t* changed_out, uint32_t* n_changed);
/* The last update call: inflation waves re-run, vertices recombined (summed over the combination nodes), |D|, incident
 * edges visited by the re-weighting (an edge between two vertices of D counts twice; 0 when edge_cost_factor == 0), device
 * milliseconds of the whole call and of its waves.  Any pointer may be NULL. */
int mnav_map_stats(const mnav_ctx* ctx, uint32_t* waves, uint32_t* recombined, uint32_t* default_changed, uint32_t* edges_reweighted,
                   float* ms_total, float* ms_wave);

/* -- replan on the resident potentials ---------------------------------------------------------
 * Brings the n plans of the last Dijkstra call (mnav_plan_dijkstra, _batch, _batch_at) up to date with the resident costs and
 * with new robot vertices (targets: n ids in the caller's order, NULL = unchanged).  Seeds and cost_limit are those of that
 * call.  Outputs, codes and the path order are those of mnav_plan_dijkstra_batch, bit for bit what a fresh plan on the
 * resident map returns; the finalize pass always runs, so dist, pred and (with mnav_set_resident_outputs) the vector maps are
 * resident afterwards and mnav_follow_batch, mnav_follow_rollout, mnav_download_output and a further replan work on them.
 * The context logs which vertices mnav_update_costs, mnav_update_edge_weights (both endpoints) and the mnav_map_* update
 * calls (the default layer's change list) touched since the last Dijkstra or replan call.  A plan keeps every value strictly
 * below its rewind level L = min(old cut, smallest old value over the closed one-ring of the logged vertices); the rest goes
 * back to +inf and the tile rounds -- or, by the option replan_repair_engine, the tile-batch engine (mnav_replan_warm_stats) --
 * continue from the kept part.  mnav_cancel is honoured between
 * chunks of rounds (the flag is cleared at entry); a cancelled call leaves nothing to replan.
 * Refused with MNAV_INTERNAL_ERROR, mnav_last_error set and outputs, log and replan state untouched: no mesh or costs, a NaN
 * offset, no Dijkstra call before, n different from that call's. */
uint32_t mnav_replan_dijkstra_batch(mnav_ctx* ctx, uint32_t n, const uint32_t* targets, double goal_dist_offset, uint32_t* codes_out,
                                    float* dist_out, uint32_t* pred_out, uint32_t* path_out, uint32_t path_cap, uint32_t* path_len);
/* The n a replan call must pass: the plans of the last Dijkstra call (0: none recorded, a replan is refused). */
uint32_t mnav_replan_plans(const mnav_ctx* ctx);
/* The last mnav_replan_dijkstra_batch.  reason: 0 the fields were repaired; otherwise the call planned afresh from the recorded
 * seeds (always a correct answer): 1 no usable resident field (the last call ran the band steps, was sharded, a CVP call,
 * failed or was cancelled, or a paths-only tile-batch call), 2 the change log ran over (option replan_log_cap, default V
 * entries) or a writer replaced whole arrays (mnav_upload_costs, mnav_compute_edge_weights, mnav_combine_*, mnav_map_compute),
 * 3 a plan of the last call never reached the device or a new target is out of range or equals its seed, 4 the option
 * replan_fresh_below = f > 0 (default 0.25, 0: never) and min over the plans with a finite old cut of L / cut < f.  log_len: logged ids at entry.
 * For reason 0: levels_out (n floats, caller's order) the rewind levels; owned vertices kept and rewound from a finite value,
 * tiles woken, summed over the plans; round launches; device milliseconds of the level kernels, the rewind, the rounds and the
 * finalize pass.  Zero otherwise (levels_out untouched).  Any pointer may be NULL. */
int mnav_replan_stats(const mnav_ctx* ctx, uint32_t* reason, uint32_t* log_len, float* levels_out, uint64_t* kept, uint64_t* rewound,
                      uint32_t* tiles_woken, uint32_t* rounds, float* ms_level, float* ms_rewind, float* ms_rounds, float* ms_finalize);

/* The replan plan by plan: arguments, outputs, refusals and the whole-call reasons 1, 2 and 3 of mnav_replan_dijkstra_batch, and
 * every output -- codes, paths, dist_out, pred_out, the resident dist / pred / vector map of every slot, the settled count --
 * is again bit for bit that of a fresh plan on the resident map.  What differs is how each plan gets there.  With L the
 * plan's rewind level, cut its old cut and f the option replan_fresh_below, the first match decides, per plan, on the device:
 *   KEPT (0)      no logged vertex has a value at or below the cut in its closed one-ring (L == cut, and no such value AT the
 *                 cut: it may belong to an expanded source), the new target is the recorded one, the offset has the recorded
 *                 bits and the resident field went through a finalize pass (the last call asked for fields or kept the
 *                 vector maps resident, or was a replan; never slot 0 after an inflation wave worked in it).  Nothing of the
 *                 plan is written; its path and settled count are read from what is resident.
 *   FRESH (2)     f > 0, the cut is finite and positive and L / cut < f: planned afresh, all FRESH plans as one batch in their
 *                 own slots, on the engine `auto` picks for their number.
 *   REPAIRED (1)  everything else: the rewind, the tile rounds and the finalize pass of mnav_replan_dijkstra_batch, over
 *                 these plans only -- or, by the option replan_repair_engine, a warm start of the tile-batch engine
 *                 (mnav_replan_warm_stats below).
 * When more than the share replan_each_fresh_share of the plans is FRESH (default 0.004, measured; 1: never) the whole call plans afresh
 * (reason 4), as it does for reasons 1 to 3.  After the call the change log starts over and mnav_follow_batch,
 * mnav_follow_rollout, the mnav_fleet_* calls, mnav_download_output and a further replan work on every slot, KEPT ones
 * included.  DESIGN.md section 3.14. */
uint32_t mnav_replan_dijkstra_each(mnav_ctx* ctx, uint32_t n, const uint32_t* targets, double goal_dist_offset, uint32_t* codes_out,
                                   float* dist_out, uint32_t* pred_out, uint32_t* path_out, uint32_t path_cap, uint32_t* path_len);
/* The last mnav_replan_dijkstra_each.  reason: as in mnav_replan_stats (4: the share policy); whole_fresh: 1 when the whole
 * call planned afresh; log_len: logged ids at entry.  Whenever the classes were taken (reason 0, and reason 4): classes_out
 * (n bytes, caller's order: 0 KEPT, 1 REPAIRED, 2 FRESH), levels_out (n floats) and counts[3] (KEPT, REPAIRED, FRESH).  For
 * reason 0: owned vertices kept and rewound from a finite value and tiles woken, summed over the REPAIRED plans; round
 * launches; fresh_engine: the value mnav_last_engine would give for the FRESH batch, -1 without one; ms[5]: device
 * milliseconds of level + classify + gather, the rewind, the rounds and the finalize pass, and host milliseconds of the FRESH
 * batch.  Any pointer may be NULL.  mnav_last_engine after a reason-0 call: 256 + 128 (tile rounds ran) + the FRESH batch's
 * engine (127: none). */
int mnav_replan_each_stats(const mnav_ctx* ctx, uint32_t* reason, uint32_t* whole_fresh, uint32_t* log_len, uint8_t* classes_out,
                           float* levels_out, uint32_t* counts, uint64_t* kept, uint64_t* rewound, uint32_t* tiles_woken, uint32_t* rounds,
                           int32_t* fresh_engine, float* ms);

/* The repaired plans on the tile-batch engine.  The plans a replan call repairs (all n of a reason-0
 * mnav_replan_dijkstra_batch, the REPAIRED class of mnav_replan_dijkstra_each) are finished either on the tile rounds or on the
 * tile-batch engine, started from the rewound fields instead of from +inf: the kernel k_tb_warm writes every slice and every
 * pending word of the sub-batch from the resident potentials and the rewind levels (same rule: the seed, and every value
 * strictly below L, is kept), and the engine's schedule, solve, finalize and path kernels run unchanged.  Outputs are the same
 * bits either way.  Options: replan_repair_engine = 0 the tile rounds, 5 the tile-batch engine whenever a plan is repaired,
 * unset automatic -- the tile-batch engine from replan_warm_min_plans repaired plans on (default 299, measured, DESIGN.md
 * section 3.14; the built-in default is never below 161, under which a fresh plan does not take that engine either).  When the engine cannot be used the
 * call falls back to the tile rounds and says so here; it never fails for that reason.
 * The last replan call of either kind: plans repaired warm (0: none, the other outputs are zero); kernel: 0 k_tb_solve_q,
 * 1 k_tbv_solve; iterations of the engine; (tile, plan) pairs woken by k_tb_warm; words: slice words it wrote; ms[3]: device
 * milliseconds of k_tb_warm, of the engine run and of k_tb_finalize; fallback: 0 none, 1 more than 65535 repaired plans, 2 the
 * engine's tables or batch state could not be allocated next to the resident outputs; live: 1 while no other planner call has
 * run since a warm repair.  Any pointer may be NULL.
 * For a warm repair mnav_replan_stats / mnav_replan_each_stats report: rounds = the engine's iterations, ms_rewind = k_tb_warm,
 * ms_rounds = the engine run, ms_finalize = k_tb_finalize, kept / rewound as always, tiles_woken = the pairs woken (tiles of the
 * tile-batch tiling).  mnav_last_engine after a per-plan call whose REPAIRED plans ran warm: 256 + 512 (+ 1024 with k_tbv_solve)
 * + the FRESH batch's engine (127: none), without the 128; after a warm mnav_replan_dijkstra_batch the tile-batch engine's
 * value (5, or 21 with k_tbv_solve). */
int mnav_replan_warm_stats(const mnav_ctx* ctx, uint32_t* plans, uint32_t* kernel, uint32_t* iterations, uint64_t* pairs_woken, uint64_t* words,
                           float* ms, uint32_t* fallback, uint32_t* live);

/* -- pose lookup on the device ---------------------------------------------------------------------
 * MeshMap::getNearestVertexHandle (mesh_map.cpp:1161-1174) and MeshMap::getContainingFace / searchContainingFace
 * (:1120-1159) for n positions (pos: n*3 floats) in one call; only the positions go up and the results come down.
 *   vertex   the minimum over ALL uploaded vertices (isolated ones included) of the pair (d, id), d = (dx*dx + dy*dy) + dz*dz
 *            in float with dx = pos.x - x_v, no contraction: the exact nearest vertex, equal d to the smallest id.  A vertex
 *            whose d is +inf or NaN never wins (so a vertex with a non-finite coordinate never does), and a position with a
 *            NaN, an infinite or an overflowing coordinate finds MNAV_NONE.
 *   face     among the faces of that vertex, in the getFacesOfVertex row order (mnav_set_face_circulation, or the library's
 *            own replay), those that pass the inside test of projectedBarycentricCoords (util.cpp:320-347, EPSILON 0.01);
 *            the smallest SIGNED plane distance wins, the first row entry on a tie; a degenerate face (NaN barycentrics) is
 *            never inside.  MNAV_NONE if there is none.
 *   bary     the three barycentric coordinates in that face, dist the signed distance; zeros without a face.
 * Any output pointer may be NULL; n = 0 does nothing.  The search structure, a linear BVH over the vertex positions of
 * O(V) bytes whatever the extent of the mesh, is built by the first call after mnav_upload_mesh and dropped by the next
 * upload; pruning compares exact lower bounds, so the result never depends on it.
 * Returns 0 / <0 (mnav_last_error; e.g. before a mesh was uploaded).  No plan output and no layer is touched. */
int mnav_locate(mnav_ctx* ctx, uint32_t n, const float* pos, uint32_t* vertex_out, uint32_t* face_out, float* bary_out,
                float* dist_out);
/* The last lookup (mnav_locate or a plan call that starts from positions): built = 1 if that call built the search
 * structure; device milliseconds of the last build and of the last query kernel; vertex distances the last call
 * evaluated, over all its positions.  Any pointer may be NULL. */
int mnav_locate_stats(const mnav_ctx* ctx, uint32_t* built, float* ms_build, float* ms_query, uint64_t* candidates);
/* MeshPlanner::makePlan's resolution (dijkstra_mesh_planner.cpp:235-236) followed by mnav_plan_dijkstra_batch: plan i runs
 * from the nearest vertex of goal_pos[i] (the wave seed) to the nearest vertex of start_pos[i] (the robot), both n*3
 * floats.  A goal without a vertex gives MNAV_INVALID_START, a start without one MNAV_INVALID_GOAL, as out-of-range ids do
 * there.  seeds_out / targets_out (n each, may be NULL) receive the resolved ids; every other argument and every output is
 * that of mnav_plan_dijkstra_batch called with those ids, bit for bit.  Only 2n ids pass through the host. */
uint32_t mnav_plan_dijkstra_batch_at(mnav_ctx* ctx, uint32_t n, const float* goal_pos, const float* start_pos,
                                     double goal_dist_offset, double cost_limit, uint32_t* codes_out, uint32_t* seeds_out,
                                     uint32_t* targets_out, float* dist_out, uint32_t* pred_out, uint32_t* path_out,
                                     uint32_t path_cap, uint32_t* path_len);
/* The same for mnav_plan_cvp_batch: seed_pos = goal_pos as given (the reference does not project it), seed face / target
 * face = the containing faces of goal_pos[i] / start_pos[i]; a position without a face gets the code an out-of-range face
 * gets there.  seed_faces_out / target_faces_out (n each, may be NULL) receive the faces. */
uint32_t mnav_plan_cvp_batch_at(mnav_ctx* ctx, uint32_t n, const float* goal_pos, const float* start_pos,
                                double goal_dist_offset, double cost_limit, uint32_t* codes_out, uint32_t* seed_faces_out,
                                uint32_t* target_faces_out, float* dist_out, uint32_t* pred_out, float* vecmap_out);

/* -- vector-field follower on the device -------------------------------------------------------------
 * One tick of mesh_controller::MeshController (computeVelocityCommands, mesh_controller.cpp:67-170, and naiveControl,
 * :225-242) for n robots over the vector maps the last plan call left resident (a single plan or a batch, Dijkstra or CVP;
 * resident through mnav_set_resident_outputs or through a vecmap_out buffer): only 44 bytes per robot go up (48 with seed_faces) and the
 * commands come down, no V-sized field crosses PCIe.  The eight parameters of mesh_controller.h:193-200: */
typedef struct mnav_follow_config {
  double max_lin_velocity;     /* 1.0 */
  double max_ang_velocity;     /* 0.5 */
  double arrival_fading;       /* 0.5; unused, as in the reference */
  double ang_vel_factor;       /* 1.0 */
  double lin_vel_factor;       /* 1.0 */
  double max_angle;            /* 20 (degrees) */
  double max_search_radius;    /* 0.4 */
  double max_search_distance;  /* 0.4 */
} mnav_follow_config;
#define MNAV_FOLLOW_CONFIG_DEFAULTS { 1.0, 0.5, 0.5, 1.0, 1.0, 20.0, 0.4, 0.4 }
/* Outcome of one robot's tick.  The ROS plugin maps them to mbf_msgs ExePath results (SUCCESS, OUT_OF_MAP, FAILURE). */
enum { MNAV_FOLLOW_OK = 0, MNAV_FOLLOW_OUT_OF_MAP = 1, MNAV_FOLLOW_NO_FIELD = 2 };
/* Robot i: position pos[i], heading dir[i] and up vector up[i] (3 floats each, in the map frame, used as given), the face
 * it was on at the last tick face_in[i] (MNAV_NONE: none yet), the plan whose field it follows slots[i] (plan index of the
 * last plan call; robots may share one) and, if seed_faces is not NULL, that plan's seed face seed_faces[i] (MNAV_NONE:
 * none), whose three vertices always count as having a vector, as in the back-tracking walk.
 *   face   in the reference's order; how_out[i] tells which step found it:
 *            1  no face_in: searchContainingFace, the rule of mnav_locate (max_search_distance is ignored there, :82-83)
 *            2  face_in still holds the position: inside and the SIGNED plane distance < max_search_distance (:109-111,
 *               no fabs: a robot far below its face stays on it); the position is kept
 *            3  searchNeighbourFaces around face_in with max_search_radius / max_search_distance (mesh_map.cpp:999-1068)
 *            4  searchContainingFace
 *            0  none: code MNAV_FOLLOW_OUT_OF_MAP (also for a position with a non-finite coordinate)
 *          in steps 1, 3 and 4 pos_out[i] is the projection v0*b0 + v1*b1 + v2*b2 (util.h:182-183), else pos[i]
 *   field  directionAtPosition (mesh_map.cpp:625-650) on the vector map; no vector at the three vertices, or a
 *          non-finite sum: code MNAV_FOLLOW_NO_FIELD (face, bary, pos and how are set, the rest is zero)
 *   mesh_dir_out  that vector divided by its float length; cost_out = c0*b0 + c1*b1 + c2*b2 over the resident vertex costs
 *   cmd_out       2 doubles per robot: linear x and angular z velocity, naiveControl in its mix of float and double, then
 *                 the two std::min saturations in double (:161-162)
 * All arithmetic is the reference's in type and order: every output equals the host's bit for bit, whichever pass of the
 * device produced it.  Not pinned (lvr2 / tf2 sources are not part of the reference): whether mesh_map::Normal's
 * constructor normalises mesh_dir a second time (here: once), and the quaternion-to-basis product of
 * poseToDirectionVector (dir / up arrive as vectors).  A neighbour search that would list more than 1024 faces goes on
 * with step 4.  Any output pointer may be NULL; n = 0 does nothing.
 * Returns 0, or -1 with mnav_last_error set and NOTHING touched: no mesh, no costs, a slot that is not a plan of the last
 * call, a slot whose vector map is not resident (also after a paths-only batch, which mnav_vector_at still serves), a
 * face id >= F that is not MNAV_NONE, a non-finite or non-positive search radius or distance.  The call changes no plan
 * output, no layer and no statistic of another entry point; it builds the lookup index of mnav_locate when a robot
 * reaches step 1 or 4 and none exists yet (mnav_locate_stats then reports built = 1).  DESIGN.md section 3.8. */
int mnav_follow_batch(mnav_ctx* ctx, uint32_t n, const float* pos, const float* dir, const float* up, const uint32_t* face_in,
                      const uint32_t* slots, const uint32_t* seed_faces, const mnav_follow_config* config, int32_t* code_out,
                      uint32_t* face_out, float* bary_out, float* pos_out, float* mesh_dir_out, float* cost_out, double* cmd_out,
                      int32_t* how_out);
/* The last mnav_follow_batch: robots that stayed on their face (how 2), found a neighbour face (3), were found by a global
 * search (1 or 4), are out of the map, have no field; built_index = 1 if the call built the lookup index; device
 * milliseconds of its kernels and host milliseconds of the whole call.  Any pointer may be NULL. */
int mnav_follow_stats(const mnav_ctx* ctx, uint32_t* stayed, uint32_t* neighbour, uint32_t* global, uint32_t* lost,
                      uint32_t* no_field, uint32_t* built_index, float* ms_kernels, float* ms_total);

/* -- device rollouts: many controller ticks per call -------------------------------------------------
 * Move Base Flex's controller loop (computeVelocityCommands, then isGoalReached, at the controller frequency until the robot
 * arrives) for n robots over `ticks` ticks, the robots' state resident and the tick loop on the device: the inputs of
 * mnav_follow_batch go up once, only the final state comes down (plus an optional strided trace of positions).  For fleets,
 * rollouts and arrival estimates over fields that cannot leave the device; a controller plugin that serves one robot keeps
 * ticking once per call through mnav_follow_batch.  Final state of a robot: */
enum { MNAV_ROLLOUT_RUNNING = 0, MNAV_ROLLOUT_REACHED = 1, MNAV_ROLLOUT_OUT_OF_MAP = 2, MNAV_ROLLOUT_NO_FIELD = 3 };
typedef struct mnav_rollout_config {
  double   dt;               /* seconds per tick */
  double   dist_tolerance;   /* isGoalReached (mesh_controller.cpp:172-177); unused without goals */
  double   angle_tolerance;
  uint32_t ticks;            /* ticks of this call, 1 .. 100000 */
  uint32_t trace_stride;     /* 0: no trace; else a position row after every trace_stride-th tick */
} mnav_rollout_config;
/* Every robot starts RUNNING with ticks = 0, travel = cost_integral = 0 and min_goal_dist = +inf.  One tick of a RUNNING
 * robot, in this order and these types (float32 / double as written, no contraction):
 *   1  R = one mnav_follow_batch tick of (pos, dir, up, face), bit for bit; ticks += 1
 *   2  R is MNAV_FOLLOW_OUT_OF_MAP: status OUT_OF_MAP, face = MNAV_NONE, pos unchanged, the robot stops
 *   3  pos = R.pos, face = R.face
 *   4  with goals: gd = |goal_pos - pos|, ang = acosf(goal_dir . dir) (the host libm's bits); min_goal_dist = min(min_goal_dist,
 *      gd); gd <= (float)dist_tolerance && ang <= (float)angle_tolerance: status REACHED, the robot stops (a NaN angle, from
 *      a dot product rounded above 1, is not reached, as in the reference)
 *   5  R is MNAV_FOLLOW_NO_FIELD: status NO_FIELD, the robot stops
 *   6  the unicycle: step = R.lin * dt (double); travel += step; cost_integral += (double)R.cost * dt;
 *      pos.c = (float)((double)pos.c + (double)dir.c * step); th = (float)(R.ang * dt); dir = the float Rodrigues rotation
 *      of dir about up by th (the host libm's cosf / sinf bits), normalised
 * A robot that is not RUNNING is left untouched by later ticks.  seed_faces may be NULL; goal_pos / goal_dir (n * 3 each) are
 * both given or both NULL (no goal test).  Outputs (any may be NULL): the final status, ticks run, position, heading and
 * face per robot, the distance travelled and the integral of the cost over time (both sums of THIS call), the smallest
 * goal distance seen, and trace_out: n * (ticks / trace_stride) * 3 floats, robot-major, row k = the position after tick
 * (k + 1) * trace_stride (a stopped robot repeats its last position).  n = 0 does nothing.
 * Resuming: pos_out, dir_out and face_out of the RUNNING robots fed back as the inputs of a second call continue the
 * rollout exactly: a + b ticks in one call or in two give the same status, position, heading and face bits.
 * mnav_cancel is honoured between blocks of at most 256 ticks (one stream synchronise and one look at the flag per block;
 * the flag is cleared at entry, as the plan calls do): the call then returns 1 and the outputs hold the state reached
 * (ticks_out tells how far; trace rows beyond it are unspecified).
 * Returns 0, 1 when cancelled, or -1 with mnav_last_error set and NOTHING touched: every refusal of mnav_follow_batch, a dt
 * that is not finite and positive, ticks outside 1 .. 100000, a trace_stride without trace_out or larger than ticks, only one
 * of goal_pos / goal_dir, a NaN tolerance, |max_ang_velocity| * max(1, |ang_vel_factor|) * dt >= 100 (the restated sinf /
 * cosf are pinned for |x| < 120 only).  The call changes no plan output, no layer and no statistic of another entry point;
 * it builds the lookup index of mnav_locate at its start if none exists yet (mnav_locate_stats then reports built = 1).
 * DESIGN.md section 3.10. */
int mnav_follow_rollout(mnav_ctx* ctx, uint32_t n, const float* pos, const float* dir, const float* up, const uint32_t* face_in,
                        const uint32_t* slots, const uint32_t* seed_faces, const float* goal_pos, const float* goal_dir,
                        const mnav_follow_config* config, const mnav_rollout_config* rollout, int32_t* status_out,
                        uint32_t* ticks_out, float* pos_out, float* dir_out, uint32_t* face_out, double* travel_out,
                        double* cost_integral_out, float* min_goal_dist_out, float* trace_out);
/* The last mnav_follow_rollout: status_counts[4] = robots per final status (indexed by MNAV_ROLLOUT_*), the robot-ticks run,
 * how they were resolved summed over all ticks (stayed on the face, neighbour search, global search; a tick that lost the
 * map is in none), built_index = 1 if the call built the lookup index, device milliseconds of its kernels and host
 * milliseconds of the whole call.  Any pointer may be NULL. */
int mnav_rollout_stats(const mnav_ctx* ctx, uint32_t* status_counts, uint64_t* robot_ticks, uint64_t* stayed, uint64_t* neighbour,
                       uint64_t* global, uint32_t* built_index, float* ms_kernels, float* ms_total);

/* -- fleet rollouts: departure ticks and a separation check between robots ----------------------------
 * mnav_follow_rollout with a start tick per robot (where mnav_fleet_schedule's departures go) and, at chosen ticks, a check
 * on the device that tells every robot whether another robot stands within a radius, which one, when and how close: what
 * a caller otherwise finds by pulling the strided trace over PCIe and searching it on the host.  The controller stays the
 * reference's: nobody reacts to a near robot. */
#define MNAV_SEP_WAITING_PRESENT 1u   /* a robot that has not departed yet stands in the way */
#define MNAV_SEP_REACHED_PRESENT 2u   /* a robot that REACHED its goal stays in the way */
typedef struct mnav_separation_config {
  double   radius;        /* used as (float)radius, > 0; r2 = (float)radius * (float)radius must be finite and > 0 */
  uint32_t check_stride;  /* a check after every check_stride-th tick of the call, 1 .. ticks */
  uint32_t flags;         /* MNAV_SEP_* or 0 */
} mnav_separation_config;
/* Inputs and outputs up to trace_out are mnav_follow_rollout's, with its rule for a tick.
 * DEPARTURE.  The ticks of a call are numbered 1 .. ticks.  start_tick: n entries, or NULL for all 0.  Robot i WAITS at tick
 * t iff t <= start_tick[i]: its status stays RUNNING, it has no controller tick, its ticks, pos, dir, face, travel,
 * cost_integral and min_goal_dist are untouched, and the trace repeats its position.  From tick start_tick[i] + 1 on it runs
 * mnav_follow_rollout's tick unchanged.  So robot i's state outputs are those of mnav_follow_rollout over
 * ticks - min(start_tick[i], ticks) ticks, its trace is that call's trace moved down by start_tick[i] rows (ticks, not
 * strides) below rows that repeat the start position, and with start_tick[i] >= ticks it comes back as it went in.  With
 * start_tick = NULL and separation = NULL every output is mnav_follow_rollout's bit for bit.  Resuming works as there; the
 * caller subtracts the ticks already run from the start ticks (saturating at 0).
 * A CHECK happens after call tick t for every t with t % check_stride == 0, on the positions as they then stand (those a
 * trace row of that tick holds).  Robot i is PRESENT at it iff its three coordinates are finite and it is RUNNING and not
 * waiting, or OUT_OF_MAP or NO_FIELD (a stranded robot is an obstacle), or waiting with MNAV_SEP_WAITING_PRESENT, or REACHED
 * with MNAV_SEP_REACHED_PRESENT.  Two present robots i != j are NEAR iff d2 <= r2, with dx = pi.x - pj.x (dy, dz alike) and
 * d2 = (dx*dx + dy*dy) + dz*dz, all float32, every operation rounded on its own (no contraction): d2 is symmetric.  The near
 * robots of i at a check are its PARTNERS.  Per robot, over the checks of this call (any pointer may be NULL; all of them
 * must be NULL when separation is NULL):
 *   near_checks_out       checks with at least one partner
 *   max_partners_out      the most partners at one check
 *   first_near_tick_out   the tick of the first check with a partner, or MNAV_NONE
 *   first_near_robot_out  at that check the partner with the smallest d2, ties to the smallest index; or MNAV_NONE
 *   min_sep2_out          the smallest d2 over all checks and partners, or +inf (only partners count: nothing beyond the
 *                         radius is measured)
 *   min_sep_tick_out      the tick of the first check that attains min_sep2, or MNAV_NONE
 *   min_sep_robot_out     at that check the partner with the smallest d2, ties to the smallest index; or MNAV_NONE
 * Counts and minima only: the same bits on every run, with any separation_cell_scale (option, 1 .. 4, the side of the search
 * grid's cells in radii).
 * THE GUARD.  Before a check compares anything the device sums T, the distance tests it would perform: over the present
 * robots, the population of the grid cells each one examines (its own cell, hence itself, included).  T depends on the
 * positions and the grid only.  T > separation_max_tests (option, default 2^32): the check is SKIPPED -- nothing is compared,
 * no robot's outputs change -- and the call goes on without asking the host.
 * mnav_cancel as in mnav_follow_rollout; the separation outputs then cover the checks run.
 * Returns 0; 1 when cancelled; 2 when the call ran to its end but at least one check was skipped; or -1 with
 * mnav_last_error set and NOTHING touched: every refusal of mnav_follow_rollout, a radius that is not positive or whose r2
 * is not finite and positive, a check_stride of 0 or above ticks, an unknown flag bit, a separation output without
 * separation, a separation_cell_scale outside 1 .. 4.  n = 0 does nothing.  The call changes no plan output, no layer and no statistic of
 * another entry point (mnav_rollout_stats keeps its values); it builds the lookup index as mnav_follow_rollout does.
 * DESIGN.md section 3.20. */
int mnav_fleet_rollout(mnav_ctx* ctx, uint32_t n, const float* pos, const float* dir, const float* up, const uint32_t* face_in,
                       const uint32_t* slots, const uint32_t* seed_faces, const float* goal_pos, const float* goal_dir,
                       const mnav_follow_config* config, const mnav_rollout_config* rollout, const uint32_t* start_tick,
                       const mnav_separation_config* separation, int32_t* status_out, uint32_t* ticks_out, float* pos_out,
                       float* dir_out, uint32_t* face_out, double* travel_out, double* cost_integral_out,
                       float* min_goal_dist_out, float* trace_out, uint32_t* near_checks_out, uint32_t* max_partners_out,
                       uint32_t* first_near_tick_out, uint32_t* first_near_robot_out, float* min_sep2_out,
                       uint32_t* min_sep_tick_out, uint32_t* min_sep_robot_out);
/* The last mnav_fleet_rollout.  status_counts .. built_index: as mnav_rollout_stats, for this call.  checks_run / _skipped and
 * the tick of the first skipped check (MNAV_NONE: none); robots with near_checks > 0; the unordered near pairs summed over
 * the checks run; the most near pairs at one check and its tick (the first such check; MNAV_NONE without a check run); the
 * smallest d2 of the call and its pair min_pair[2] = (i, j), i < j (+inf and MNAV_NONE twice without a near pair); the
 * distance tests performed (the T of every check run); the largest cell population met; device milliseconds of the
 * separation kernels, of all kernels, and host milliseconds of the whole call.  Any pointer may be NULL. */
int mnav_fleet_rollout_stats(const mnav_ctx* ctx, uint32_t* status_counts, uint64_t* robot_ticks, uint64_t* stayed,
                             uint64_t* neighbour, uint64_t* global, uint32_t* built_index, uint32_t* checks_run,
                             uint32_t* checks_skipped, uint32_t* first_skipped_tick, uint32_t* robots_near, uint64_t* near_pairs,
                             uint64_t* max_pairs, uint32_t* max_pairs_tick, float* min_sep2, uint32_t* min_pair, uint64_t* tests,
                             uint32_t* max_cell, float* ms_separation, float* ms_kernels, float* ms_total);

/* -- fleet rollouts in which robots yield: right of way, decided inside the check ------------------------
 * mnav_fleet_rollout reports near robots and nobody reacts.  mnav_fleet_rollout_yield evaluates a right-of-way rule inside the
 * same check, on the device: a robot that has to yield has no controller tick until the next check, so followers queue
 * behind the robot ahead instead of driving through it, and arrival ticks, travel and cost integrals are those of robots
 * that share the mesh.  The rule is stateless per check and made of compares, counts and minima: the same bits on every
 * run, with any separation_cell_scale. */
typedef struct mnav_yield_config {
  double   ahead_cos;   /* used as c = (float)ahead_cos, finite, 0 <= c < 1: the cosine of the half angle of the cone "ahead";
                           c2 = c * c in float32 */
  uint32_t flags;       /* reserved, must be 0 */
} mnav_yield_config;
/* Every argument up to min_sep_robot_out is mnav_fleet_rollout's, in its order and with its meaning; then the yield group.
 * YIELD IS NULL.  Then priority, hold_in, hold_out and the four yield outputs must be NULL too, every output is
 * mnav_fleet_rollout's bit for bit, and the call launches the very kernels that call launches.
 * YIELD IS GIVEN.  separation must be given: the rule uses its radius, check_stride and presence flags, and the separation
 * outputs are what mnav_fleet_rollout would report for the motion that results.
 * TERMS at the check after call tick t (t % check_stride == 0), on positions, headings, statuses, start ticks and priorities
 * as they stand after tick t:
 *   robot i is a MOVER iff its status is RUNNING and it is not waiting (t > start_tick[i]);
 *   a PARTNER of i is what it is in mnav_fleet_rollout: a present robot j != i with d2 <= r2, d2 the float32 sum defined there;
 *   A(i, j), "j is AHEAD of i": ex = pj.x - pi.x (ey, ez alike), dot = (dir_i.x*ex + dir_i.y*ey) + dir_i.z*ez,
 *     A = dot > 0 && dot*dot >= c2*d2, all float32, every operation rounded on its own (no contraction), d2 the pair's d2
 *     above.  A NaN anywhere gives false (a NaN heading sees nobody ahead).  Coincident robots have dot == 0: they are ahead
 *     of nobody;
 *   before(j, i) iff (priority[j], j) < (priority[i], i) lexicographically.  priority: n entries, or NULL for all equal, so
 *     that the index decides.  A smaller priority value has right of way.
 * THE DECISION.  A present mover i YIELDS TO its partner j iff
 *     j is not a mover (stranded, or waiting or REACHED and kept present by a flag) and A(i, j), or
 *     j is a mover and A(i, j) && (!A(j, i) || before(j, i)).
 * A follower yields to whoever drives ahead of it, whatever the priorities; of two robots that face each other the one
 * without right of way yields; robots side by side do not yield.  hold[i] = 1 iff i is a present mover and yields to at
 * least one partner, else 0.  The decision never reads the flags of the check before, so within a check it cannot
 * oscillate, and a check depends on nothing but the state after its tick.  A check that the guard skips sets every hold to
 * 0: with no information nobody is held.
 * THE TICK.  At call tick t robot i has a controller tick iff it is RUNNING, not waiting, and hold[i] == 0, where hold is
 * hold_in (n bytes, NULL for all 0; any non-zero byte is 1) until the first check of the call and afterwards what the latest
 * check left.  A held robot is treated like a waiting one: its ticks, pos, dir, face, travel, cost_integral and
 * min_goal_dist are untouched and the trace repeats its position.
 * Per robot, over this call (any pointer may be NULL; all of them must be NULL when yield is NULL):
 *   hold_checks_out       checks that left it held
 *   held_ticks_out        call ticks at which it was RUNNING, not waiting and held
 *   first_hold_tick_out   the tick of the first check that held it, or MNAV_NONE
 *   first_hold_robot_out  its BLOCKER at that check: the yielded-to partner with the smallest d2, ties to the smallest index;
 *                         or MNAV_NONE
 *   hold_out              n bytes, 0 or 1: the flags after the last check of the call (hold_in as flags if no check ran)
 * RESUMING works as in mnav_fleet_rollout -- the RUNNING robots' pos_out, dir_out and face_out back in, the start ticks
 * reduced by the ticks already run -- with those robots' hold_out fed back as hold_in.  The second call continues the first
 * exactly (the state bits of one call of a + b ticks; hold_checks and held_ticks add up) when the first call's tick count a
 * is a multiple of check_stride -- its last tick then had a check, the flags are that check's, and the checks of the second
 * call fall on the ticks they fall on in one call -- and no robot left out was present in a later check (a stopped robot
 * that is not fed back stands in nobody's way any more).
 * WHAT THE RULE DOES NOT PROMISE.  It is right of way, not avoidance: the velocity command is never changed, and a robot with
 * right of way drives on, into a held robot if that is where its field leads.  A ring of followers, each behind the next, can
 * hold each other for good; this call does not resolve that deadlock, mnav_fleet_yield_stats shows it (robots held after the
 * last check, held robot-ticks).  mnav_fleet_rollout_rings, below, tells such rings from harmless queues and releases them.
 * Returns 0, 1 and 2 as mnav_fleet_rollout, or -1 with mnav_last_error set and NOTHING touched: every refusal of
 * mnav_fleet_rollout, yield given without separation, an ahead_cos whose float is not finite or outside 0 <= c < 1, a non-zero
 * flag, priority, hold_in, hold_out or a yield output given without yield.  n = 0 does nothing.  The call has statistics
 * records of its own: it leaves mnav_rollout_stats and mnav_fleet_rollout_stats as they were, and those calls leave
 * mnav_fleet_yield_stats.  DESIGN.md section 3.21. */
int mnav_fleet_rollout_yield(mnav_ctx* ctx, uint32_t n, const float* pos, const float* dir, const float* up, const uint32_t* face_in,
                             const uint32_t* slots, const uint32_t* seed_faces, const float* goal_pos, const float* goal_dir,
                             const mnav_follow_config* config, const mnav_rollout_config* rollout, const uint32_t* start_tick,
                             const mnav_separation_config* separation, int32_t* status_out, uint32_t* ticks_out, float* pos_out,
                             float* dir_out, uint32_t* face_out, double* travel_out, double* cost_integral_out,
                             float* min_goal_dist_out, float* trace_out, uint32_t* near_checks_out, uint32_t* max_partners_out,
                             uint32_t* first_near_tick_out, uint32_t* first_near_robot_out, float* min_sep2_out,
                             uint32_t* min_sep_tick_out, uint32_t* min_sep_robot_out, const mnav_yield_config* yield,
                             const uint32_t* priority, const uint8_t* hold_in, uint8_t* hold_out, uint32_t* hold_checks_out,
                             uint32_t* held_ticks_out, uint32_t* first_hold_tick_out, uint32_t* first_hold_robot_out);
/* The last mnav_fleet_rollout_yield: robots with hold_checks > 0; the sum of held_ticks over the robots; the most robots one
 * check held and that check's tick (the first such check among those run; 0 and MNAV_NONE without a check run; a skipped
 * check holds nobody and is no candidate); the robots held after the last check (the set bytes of hold_out); the checks
 * run and skipped and the tick of the first skipped check (MNAV_NONE: none), as mnav_fleet_rollout_stats counts them; device
 * milliseconds of the pair passes (the kernel that decides), of all kernels of the checks, of all kernels, and host
 * milliseconds of the whole call.  All 0 / MNAV_NONE after a call with yield = NULL, except the times.  Any pointer may be
 * NULL. */
int mnav_fleet_yield_stats(const mnav_ctx* ctx, uint32_t* robots_held, uint64_t* held_ticks, uint32_t* max_held, uint32_t* max_held_tick,
                           uint32_t* held_last, uint32_t* checks_run, uint32_t* checks_skipped, uint32_t* first_skipped_tick, float* ms_pair, float* ms_separation, float* ms_kernels, float* ms_total);

/* -- wait-for analysis of a yielding fleet rollout: why a robot is held, rings found and released ---------
 * mnav_fleet_rollout_yield holds robots and cannot say why.  Three cases look alike in its outputs: a stop-and-go queue behind
 * a robot that still drives, a queue behind a robot that stands for good where a presence flag keeps it, and a ring of robots
 * that wait for each other -- a deadlock.  mnav_fleet_rollout_rings classifies every held robot at every check, on the device,
 * and can release one robot of every ring. */
#define MNAV_RING_RELEASE 1u      /* the leader of every ring is released at the check that finds the ring */
typedef struct mnav_ring_config {
  uint32_t flags;       /* MNAV_RING_* or 0 */
} mnav_ring_config;
#define MNAV_WAIT_FREE        0u  /* not held by the rule at that check */
#define MNAV_WAIT_QUEUED      1u  /* its chain ends at a robot that is not held and is a MOVER */
#define MNAV_WAIT_PARKED      2u  /* its chain ends at a robot that is not held and is no mover */
#define MNAV_WAIT_RING_TAIL   3u  /* its chain runs into a ring it is not part of */
#define MNAV_WAIT_RING_MEMBER 4u  /* it lies on a ring */
/* Every argument up to first_hold_robot_out is mnav_fleet_rollout_yield's, in its order and with its meaning; then the ring group.
 * RINGS IS NULL.  Then the six ring outputs must be NULL too, every output is mnav_fleet_rollout_yield's bit for bit, and the
 * call launches the very kernels that call launches.
 * RINGS IS GIVEN.  yield (and so separation) must be given.  With flags = 0 the state, the trace, the separation outputs and
 * the yield outputs are mnav_fleet_rollout_yield's bit for bit; only the ring outputs are new.
 * THE RULE applies at a check that ran, after the decision of mnav_fleet_rollout_yield:
 *   hold0[i] is the flag the right-of-way rule gives robot i;
 *   b[i] is robot i's BLOCKER at this check: the yielded-to partner with the smallest d2, ties to the smallest index -- the
 *     definition of first_hold_robot_out, applied at every check;
 *   w(i) = b[i] if hold0[i], else i.
 * b[i] != i, and b[i] is present.  Two robots never yield to each other: A(i, j) && A(j, i) would need before(j, i) &&
 * before(i, j), and a robot that is no mover is never held.  So every cycle of w other than a fixed point has at least three
 * robots: the smallest ring is a triangle.
 * The CHAIN of i is i, w(i), w(w(i)), ...  It ends at a fixed point, or it enters a cycle.  The fixed point is its ROOT, a robot
 * that is not held.  A RING is a cycle.  A ring's LEADER is its member with the smallest (priority, index), the order of before.
 * The CLASS of robot i is MNAV_WAIT_FREE if !hold0[i]; MNAV_WAIT_QUEUED if its chain ends at a root that is a mover at this
 * check; MNAV_WAIT_PARKED if it ends at a root that is no mover (waiting, REACHED or stranded, kept present); MNAV_WAIT_RING_MEMBER
 * if i lies on a ring; MNAV_WAIT_RING_TAIL if its chain enters a ring i is not part of.  anchor[i] is the root for QUEUED and
 * PARKED, the ring's leader for RING_TAIL and RING_MEMBER, MNAV_NONE for FREE.
 * The analysis follows the nearest blocker only.  A robot may yield to more partners; the classes describe that one graph.
 * RELEASE, with MNAV_RING_RELEASE: after the classification hold[leader] = 0 for every ring, every other flag is hold0.  The
 * released robot has controller ticks until the next check, whatever else it yielded to; tails and the other members stay
 * held.  Without the flag hold = hold0.  The check stays a function of the state after its tick and reads no flag of the check
 * before: nothing oscillates within a check, and every run and every separation_cell_scale gives the same bits.
 * A check that the guard skips leaves every class FREE, every anchor MNAV_NONE, and counts nothing.
 * Per robot, over the checks of this call (any pointer may be NULL; all of them must be NULL when rings is NULL):
 *   wait_class_out        n bytes: the class at the last check of the call (FREE if no check ran)
 *   wait_anchor_out       the anchor at the last check of the call (MNAV_NONE if no check ran)
 *   ring_checks_out       checks at which the robot was RING_MEMBER
 *   first_ring_tick_out   the tick of the first such check, or MNAV_NONE
 *   parked_checks_out     checks at which the robot was PARKED
 *   released_checks_out   checks at which it was released as a leader
 * THE YIELD OUTPUTS UNDER RELEASE.  hold_checks_out and first_hold_tick_out / first_hold_robot_out count the checks at which
 * the rule held the robot (hold0), released or not.  held_ticks_out and hold_out follow the flags as they stand after the
 * release, and so do the robots held after the last check.
 * RESUMING works through hold_out -> hold_in exactly as in mnav_fleet_rollout_yield; nothing new is fed back.
 * Returns 0, 1 and 2 as mnav_fleet_rollout_yield, or -1 with mnav_last_error set and NOTHING touched: every refusal of
 * mnav_fleet_rollout_yield, rings given without yield, an unknown ring flag bit, a ring output given without rings.  The
 * call has a statistics record of its own (mnav_fleet_ring_stats): it leaves mnav_rollout_stats, mnav_fleet_rollout_stats and
 * mnav_fleet_yield_stats as they were, and those calls leave mnav_fleet_ring_stats.  DESIGN.md section 3.22. */
int mnav_fleet_rollout_rings(mnav_ctx* ctx, uint32_t n, const float* pos, const float* dir, const float* up, const uint32_t* face_in,
                             const uint32_t* slots, const uint32_t* seed_faces, const float* goal_pos, const float* goal_dir,
                             const mnav_follow_config* config, const mnav_rollout_config* rollout, const uint32_t* start_tick,
                             const mnav_separation_config* separation, int32_t* status_out, uint32_t* ticks_out, float* pos_out,
                             float* dir_out, uint32_t* face_out, double* travel_out, double* cost_integral_out,
                             float* min_goal_dist_out, float* trace_out, uint32_t* near_checks_out, uint32_t* max_partners_out,
                             uint32_t* first_near_tick_out, uint32_t* first_near_robot_out, float* min_sep2_out,
                             uint32_t* min_sep_tick_out, uint32_t* min_sep_robot_out, const mnav_yield_config* yield,
                             const uint32_t* priority, const uint8_t* hold_in, uint8_t* hold_out, uint32_t* hold_checks_out,
                             uint32_t* held_ticks_out, uint32_t* first_hold_tick_out, uint32_t* first_hold_robot_out,
                             const mnav_ring_config* rings, uint8_t* wait_class_out, uint32_t* wait_anchor_out, uint32_t* ring_checks_out,
                             uint32_t* first_ring_tick_out, uint32_t* parked_checks_out, uint32_t* released_checks_out);
/* The last mnav_fleet_rollout_rings: robots with ring_checks > 0; the rings summed over the checks run; the most rings at one
 * check and that check's tick (the first such check among those run; 0 and MNAV_NONE without a check run); the releases summed
 * over the checks; RING_MEMBER, RING_TAIL, PARKED and QUEUED robots and rings at the last check of the call (all 0 when the
 * guard skipped it or no check ran); the checks run and skipped and the tick of the first skipped check, as
 * mnav_fleet_rollout_stats counts them; device milliseconds of the kernels of the analysis behind the pair passes, of all
 * kernels of the checks, of all kernels, and host milliseconds of the whole call.  All 0 / MNAV_NONE after a call with
 * rings = NULL, except the times.  Any pointer may be NULL. */
int mnav_fleet_ring_stats(const mnav_ctx* ctx, uint32_t* robots_ring, uint64_t* rings, uint32_t* max_rings, uint32_t* max_rings_tick,
                          uint64_t* releases, uint32_t* members_last, uint32_t* tails_last, uint32_t* parked_last, uint32_t* queued_last,
                          uint32_t* rings_last, uint32_t* checks_run, uint32_t* checks_skipped, uint32_t* first_skipped_tick,
                          float* ms_ring, float* ms_separation, float* ms_kernels, float* ms_total);

/* -- sampled rollouts: K candidate controls per robot, scored on the device ----------------------------
 * What a local planner asks at every control tick -- of K ways to steer for the next `ticks` ticks, which one ends lowest on
 * the potential field, at the least cost, without leaving the mesh or crossing a lethal region (DWA or MPPI over the
 * planner's own field) -- answered over the resident fields.  The robots go up as for mnav_follow_rollout, with a table
 * of n_candidates candidates shared by all robots; the device expands them into n * K rows (row i * K + k: robot i under
 * candidate k), runs every row for rollout->ticks ticks, scores every row and picks per robot.  Only the picks come down,
 * and the per-row outputs a caller asks for: nothing V-sized crosses PCIe. */
typedef struct mnav_sample_config {
  double   w_potential;   /* weights of J, each finite and >= 0 */
  double   w_cost;
  double   w_time;
  double   lethal_cost;   /* used as (float)lethal_cost; not NaN; +inf: only a NaN cost is lethal */
  uint32_t flags;         /* reserved, must be 0 */
} mnav_sample_config;
#define MNAV_SAMPLE_CONFIG_DEFAULTS { 1.0, 0.0, 0.0, 1.0, 0u }
/* candidates: 4 doubles per candidate, lin_gain, lin_bias, ang_gain, ang_bias.  Gain 0 is a constant arc (DWA), (1, 0, 1, 0)
 * is the follower itself, gain 1 with an angular bias is "follow the field but keep left".
 * Every row starts as a robot of mnav_follow_rollout, with pot = +inf, lethal = 0 and cmd0 = (0, 0).  ONE TICK OF A RUNNING
 * ROW is steps 1 to 6 of mnav_follow_rollout, same types and order, no contraction, with three differences:
 *   a  POTENTIAL AND LETHAL FLAG.  After step 3 (R is OK or NO_FIELD; the face and R.bary are known):
 *        pot = d[v0]*b0 + d[v1]*b1 + d[v2]*b2 in float, left to right (the form of cost_out of mnav_follow_batch), d the
 *        slot's resident potential -- bit for bit what mnav_download_output(slot, 0) returns --, v0..2 the face's vertices in
 *        stored order; and when R is OK: lethal |= !(R.cost < (float)lethal_cost), so a NaN cost counts as lethal
 *   b  COMMAND.  Step 6 runs under u in place of R.lin, and the same for ang:
 *        u = gain * R.lin; if (bias != 0) u += bias; u = u < max_lin_velocity ? u : max_lin_velocity
 *        (max_ang_velocity for ang: the saturation of the follower, idempotent on its own command).  A zero bias is not
 *        added -- x + 0.0 would turn -0 into +0 --, so (1, 0, 1, 0) passes R.lin and R.ang through bit for bit.  The first
 *        tick of a row that reaches step 6 records cmd0 = (u_lin, u_ang)
 *   c  END OF THE CALL.  J = w_potential * (double)pot + w_cost * cost_integral + w_time * ((double)ticks_run * dt), in
 *        double, left to right.  A row is FEASIBLE iff its status is RUNNING or REACHED, it is not lethal and J is finite
 *        (an infinite or NaN potential makes J non-finite; a row that never reached step 3 keeps pot = +inf)
 * pot is the potential where the row's LAST tick found it, that is before that tick's step: a caller who wants the
 * potential one step further asks for one more tick.
 * THE PICK, per robot: the feasible row with the smallest (J, k) -- J compared with <, ties to the smallest k, -0 ties with
 * +0.  best_k_out[i] = that k (MNAV_NONE: no row is feasible), best_score_out[i] = its J (+inf), best_cmd_out[2 i], [2 i + 1] =
 * its cmd0 (zeros), n_feasible_out[i] = the robot's feasible rows.  Optional per-row outputs, n * K each, row-major as above
 * (any may be NULL, and is then not downloaded): status, ticks, score J, potential, lethal flag (0 / 1), cost integral,
 * travel, end position (3 floats).  The pick is built from compares, counts and minima only: the same bits on every run.
 * mnav_cancel is honoured between blocks of at most 256 ticks, as in the rollouts, but the flag is NOT cleared at entry: a
 * cancel that arrived before the call ends it before its first tick (the statistics are then all 0).  A cancelled call
 * returns 1, writes no output and takes the flag down.
 * Returns 0, 1 when cancelled, or -1 with mnav_last_error set and NOTHING touched (every refusal comes before the first
 * device call): every refusal of mnav_follow_rollout, a non-zero trace_stride, n_candidates = 0 or a NULL table, a gain or
 * bias that is not finite, a weight that is negative or not finite, a NaN lethal_cost, non-zero flags, a NULL sample,
 * n * n_candidates above 2^28, a slot whose potential is not resident, a table whose largest |ang_gain| * |max_ang_velocity| *
 * max(1, |ang_vel_factor|) + |ang_bias|, times dt, reaches 100 rad.  n = 0 does nothing.  The call changes no plan output, no
 * layer and no statistic or record of another entry point (mnav_rollout_stats and the mnav_fleet_*_stats keep their values);
 * it builds the lookup index as mnav_follow_rollout does.  About 100 bytes per row stay resident.  DESIGN.md section 3.23. */
int mnav_follow_sample(mnav_ctx* ctx, uint32_t n, const float* pos, const float* dir, const float* up, const uint32_t* face_in,
                       const uint32_t* slots, const uint32_t* seed_faces, const float* goal_pos, const float* goal_dir,
                       const mnav_follow_config* config, const mnav_rollout_config* rollout, uint32_t n_candidates,
                       const double* candidates, const mnav_sample_config* sample, uint32_t* best_k_out, double* best_score_out,
                       double* best_cmd_out, uint32_t* n_feasible_out, int32_t* status_out, uint32_t* ticks_out, double* score_out,
                       float* potential_out, uint8_t* lethal_out, double* cost_integral_out, double* travel_out, float* pos_out);
/* The last mnav_follow_sample: status_counts[4] = rows per final status, lethal and feasible rows, robots without a pick, the
 * row-ticks run and how they were resolved (stayed, neighbour, global: as mnav_rollout_stats), built_index, device
 * milliseconds of the expand kernel, of the score and pick kernels, of all kernels, and host milliseconds of the whole
 * call.  After a cancelled call the three pick counts are 0.  Any pointer may be NULL. */
int mnav_sample_stats(const mnav_ctx* ctx, uint32_t* status_counts, uint32_t* lethal_rows, uint32_t* feasible_rows,
                      uint32_t* robots_without_pick, uint64_t* row_ticks, uint64_t* stayed, uint64_t* neighbour, uint64_t* global,
                      uint32_t* built_index, float* ms_expand, float* ms_pick, float* ms_kernels, float* ms_total);

/* -- fleet paths and walks: many robots per resident field ---------------------------------------------
 * A Dijkstra call returns one vertex path per plan, from the plan's seed (the goal) to its one target.  The field is seeded
 * at the goal, so it already holds the path of every robot inside it: mnav_fleet_paths hands Move Base Flex's setPlan a
 * vertex path for n robots over the fields the last Dijkstra call (mnav_plan_dijkstra, _batch, _batch_at) or the last
 * mnav_replan_dijkstra_batch left resident, without another wave and without a V-sized array crossing PCIe. */
#define MNAV_BEYOND_FIELD 70u   /* not an mbf code: the resident field cannot answer for this robot; plan or replan */
/* Robot i uses plan slots[i] (plan index of that call; robots may share one) and stands on vertex start_vertex[i] or, when
 * start_vertex is NULL, on the vertex nearest to start_pos[i] by the rule of mnav_locate (the ids stay on the device).
 * With d / p the plan's resident dist / pred, g its seed, t its target, offset and cost_limit those of the call and
 * cut = float(d[t] + offset) (d[t] itself when that rounds below d[t]; +inf when d[t] is), the first match decides:
 *   1  v >= V (an id out of range, MNAV_NONE, a position without a vertex): MNAV_INVALID_GOAL, as in mnav_plan_dijkstra_batch_at
 *   2  the plan never reached the device (rejected ids, seed == target): the plan's own code, length 0
 *      CAUTION: a plan whose seed is its target never runs and its own code is MNAV_SUCCESS, so EVERY robot on that slot gets
 *      MNAV_SUCCESS with length 0 wherever it stands; only a robot on the seed has reached the goal.  Such a robot is told
 *      apart by potential_out == +inf (rule 3 gives 0): check it, or put no robot other than the plan's own on such a slot
 *   3  v == g: MNAV_SUCCESS, length 0, potential 0
 *   4  d[v] < cut, or v == t: p[v] == v: MNAV_NO_PATH_FOUND; otherwise MNAV_SUCCESS, the path p[v], p[p[v]], ..., g written
 *      in the reference's list order (seed first ... pred[v]) and potential_out[i] = d[v]; a chain that does not reach g
 *      within V hops: MNAV_INTERNAL_ERROR
 *   5  d[v] == +inf and the wave ran out (cut == +inf, or no vertex of the plan holds a finite value at or above the cut, so
 *      every vertex the wave reached was expanded): MNAV_NO_PATH_FOUND, v is not connected to g
 *   6  otherwise MNAV_BEYOND_FIELD, length 0: the tentative ring at or above the cut and the vertices the wave never
 *      reached before it stopped; the caller plans for this robot, or replans with a larger offset
 * For every robot that gets MNAV_SUCCESS or MNAV_NO_PATH_FOUND by rules 4 and 5 the code, the ids and the potential are bit
 * for bit what mnav_plan_dijkstra_batch(seed = g, target = v) returns with the recorded offset and cost_limit on the
 * resident map.  The call may say MNAV_BEYOND_FIELD where a fresh plan would succeed; it never
 * returns another path than the fresh plan's.  potential_out is +inf wherever rules 3 and 4 do not set it.
 * Output: paths packed back to back; offset_out (n + 1) = the exclusive prefix sum of len_out in robot order,
 * offset_out[n] = *total_out; robot i's ids are ids_out[offset_out[i] .. offset_out[i] + len_out[i]).  vertex_out: the
 * vertex each robot was given or found on.  Any output pointer may be NULL; n = 0 does nothing.
 * Returns 0 when everything was written; 1 when *total_out > ids_cap or ids_out is NULL: all per-robot outputs and
 * total_out are valid then and ids_out is untouched -- size the buffer and call again; -1 with mnav_last_error set and
 * NOTHING touched: no mesh or costs, the last plan call was not a Dijkstra call or replan, a slot that is not a plan of
 * it, a slot whose predecessors are not resident (a paths-only call: mnav_device_output(slot, 1) == NULL; a sharded,
 * failed or cancelled call; the band-step engine, whose predecessors are not pinned), neither start_vertex nor
 * start_pos, or a cost-changing call since the plan (the replan's change log is not empty, or a writer replaced whole
 * arrays): the field no longer belongs to the resident map -- replan first.  The call changes no plan output, no layer
 * and no statistic of another entry point; with positions it builds the lookup index of mnav_locate when none exists
 * yet (mnav_locate_stats then reports built = 1). */
int mnav_fleet_paths(mnav_ctx* ctx, uint32_t n, const uint32_t* slots, const uint32_t* start_vertex, const float* start_pos,
                     uint32_t* code_out, uint32_t* vertex_out, float* potential_out, uint32_t* len_out, uint64_t* offset_out,
                     uint32_t* ids_out, uint64_t ids_cap, uint64_t* total_out);
/* The walk of mnav_backtrack_cvp_batch for many robots per field: robot i walks over the vector map resident for plan
 * slots[i] of the last plan call (CVP or Dijkstra, the rule of mnav_follow_batch) from start_pos[i] on start_faces[i]
 * (start_faces NULL: the containing face by the rule of mnav_locate; start_face_out receives the faces used) to
 * seed_pos[slots[i]] on seed_faces[slots[i]].  n_plans must equal the plan count of the last call.  status_out[i]: 1, 0,
 * -1, -2 as in mnav_backtrack_cvp_batch (reached; no path, also when walk_cap is hit; a vertex without an inflation
 * entry; internal list overflow); -3: no face at the
 * start (MNAV_NONE, or a position without one), length 0; 0 with length 0: a plan that never reached the device.  Rows
 * come out seed first and packed (3 floats in positions_out and one id in faces_out per entry), offset_out / total_out
 * and the return values 0 / 1 (entries_cap too small, or positions_out and faces_out both NULL) as in mnav_fleet_paths.
 * Robots are walked in chunks whose scratch rows of walk_cap entries stay within the option fleet_scratch_mb (default
 * 256 MiB); the result does not depend on it, and walk_cap * n is not bounded.
 * Returns -1 with mnav_last_error set and NOTHING touched: no mesh, a null slots / seed / start_pos array, walk_cap
 * outside 2 .. 2^24, a step_width that is not positive, n_plans different from the last call's, a slot out of range, a
 * used slot whose vector map is not resident or whose seed face is out of range, a start face >= F that is not
 * MNAV_NONE, an inflation_layer >= 0 that is no resident inflation layer with a vector field. */
int mnav_fleet_walks(mnav_ctx* ctx, uint32_t n, const uint32_t* slots, uint32_t n_plans, const float* seed_pos,
                     const uint32_t* seed_faces, const float* start_pos, const uint32_t* start_faces, double step_width,
                     int32_t inflation_layer, uint32_t walk_cap, int32_t* status_out, uint32_t* start_face_out, uint32_t* len_out,
                     uint64_t* offset_out, float* positions_out, uint32_t* faces_out, uint64_t entries_cap, uint64_t* total_out);
/* -- fleet plans: MeshPlanner::makePlan's pose list and cost for many robots per resident field ---------
 * makePlan returns neither vertex ids nor (position, face) pairs but std::vector<PoseStamped> and a cost.  The two calls
 * below turn the paths of mnav_fleet_paths and the walks of mnav_fleet_walks into exactly that on the device: 7 doubles per
 * pose (x y z qx qy qz qw) by mesh_map::calculatePoseFromPosition (util.cpp:267-298: the basis in float, the tf2
 * getRotation quaternion and its normalisation in double), bit for bit what the host loops of mnav_planner_host.hpp
 * (vertex_path_poses, face_path_poses) compute.  A pose whose direction is zero or parallel to its normal has a NaN
 * quaternion with an exact position and an exact length, as in the reference. */
/* MeshMap::faceNormals(): F * 3 floats, resident until the next mnav_upload_mesh.  Only mnav_fleet_walk_plans needs them.
 * Returns -1 with mnav_last_error set: no mesh, F different from the resident mesh's, a null array. */
int mnav_upload_face_normals(mnav_ctx* ctx, uint32_t F, const float* face_normals);
/* DijkstraMeshPlanner::makePlan's plan and cost (dijkstra_mesh_planner.cpp:83-116) for n robots over the resident fields.
 * slots, start_vertex, code_out, vertex_out, potential_out: as in mnav_fleet_paths, with the same values for the same
 * slots and vertices.  start_pos (n * 3, required): the robot position of the first pose; start_vertex may be NULL, the
 * vertex then comes from start_pos by the rule of mnav_locate.  goal_pos (n_plans * 3): the goal position of every plan
 * (the last pose looks at it); n_plans must equal the plan count of the recorded call.
 * With u_0 .. u_{L-1} that robot's path, robot side first (the reverse of the ids of mnav_fleet_paths: u_0 = pred[v],
 * u_{L-1} = the seed), xyz the vertex positions and vn the vertex normals of mnav_upload_mesh:
 *   L == 0 (any code): no poses, cost 0
 *   L > 0: L + 1 poses: pose 0 = pose_from(start_pos, xyz[u_0], vn[u_0]); pose k = pose_from(xyz[u_{k-1}], xyz[u_k],
 *          vn[u_{k-1}]) for 1 <= k < L; pose L = pose_from(xyz[u_{L-1}], goal_pos[slot], vn[u_{L-1}])
 * cost_out[i]: the double sum of the L + 1 float lengths in that order.  len_out counts poses; offset_out (n + 1) and
 * total_out as in mnav_fleet_paths, in poses; poses_out: 7 doubles per pose, packed in robot order.
 * Returns 0 when everything was written; 1 when *total_out > poses_cap or poses_out is NULL: all per-robot outputs (the
 * costs too) and total_out are valid and poses_out is untouched; -1 with mnav_last_error set and NOTHING touched: every
 * refusal of mnav_fleet_paths, vertex normals not resident, start_pos or goal_pos NULL, n_plans different from the
 * recorded call's.  Path ids (4 bytes per hop) and lengths stay in device scratch; only the caller's outputs cross PCIe. */
int mnav_fleet_plans(mnav_ctx* ctx, uint32_t n, const uint32_t* slots, const uint32_t* start_vertex, const float* start_pos,
                     uint32_t n_plans, const float* goal_pos, uint32_t* code_out, uint32_t* vertex_out, float* potential_out,
                     uint32_t* len_out, uint64_t* offset_out, double* cost_out, double* poses_out, uint64_t poses_cap,
                     uint64_t* total_out);
/* CVPMeshPlanner::makePlan's plan and cost (cvp_mesh_planner.cpp:93-124) over the walks of mnav_fleet_walks: arguments,
 * statuses, chunking (fleet_scratch_mb) and refusals are that call's, plus two refusals: face normals not resident
 * (mnav_upload_face_normals), goal_pose NULL.  goal_pose: n_plans * 7 doubles.  A row of m entries (p_0, f_0) ..
 * (p_{m-1}, f_{m-1}), seed first, whatever its status (the reference poses a partial path too), with fn the face normals:
 *   m == 0: no poses, cost 0
 *   otherwise m poses: pose k = pose_from(p_{m-1-k}, p_{m-2-k}, fn[f_{m-1-k}]) for k < m - 1; pose m - 1 = the 7 doubles
 *   of goal_pose[slot], bit for bit; cost_out[i] = the ordered double sum of the m - 1 lengths
 * len_out, offset_out, total_out count poses; return values as in mnav_fleet_plans. */
int mnav_fleet_walk_plans(mnav_ctx* ctx, uint32_t n, const uint32_t* slots, uint32_t n_plans, const float* seed_pos,
                          const uint32_t* seed_faces, const double* goal_pose, const float* start_pos, const uint32_t* start_faces,
                          double step_width, int32_t inflation_layer, uint32_t walk_cap, int32_t* status_out,
                          uint32_t* start_face_out, uint32_t* len_out, uint64_t* offset_out, double* cost_out, double* poses_out,
                          uint64_t poses_cap, uint64_t* total_out);
/* The last mnav_fleet_paths, mnav_fleet_walks, mnav_fleet_plans or mnav_fleet_walk_plans (entries: poses for the last two);
 * robots served (MNAV_SUCCESS / status 1), beyond the field, without a path
 * (MNAV_NO_PATH_FOUND / every other walk status but -3) and invalid (every other code / status -3); path ids or walk
 * entries summed; built_index = 1 if the call built the lookup index; chunks of a walk call; device milliseconds of its
 * kernels and host milliseconds of the whole call.  Any pointer may be NULL. */
int mnav_fleet_stats(const mnav_ctx* ctx, uint32_t* served, uint32_t* beyond_field, uint32_t* no_path, uint32_t* invalid,
                     uint64_t* entries, uint32_t* built_index, uint32_t* chunks, float* ms_kernels, float* ms_total);

/* -- fleet dispatch: which goal does each robot go to? ------------------------------------------------
 * Every fleet call above takes slots[i], the goal of robot i, as an input.  With K goal fields resident and R robots the
 * cost of robot r to reach goal k is one float, d_k[v_r]; the two calls below compute the R x K matrix of them on the
 * device and an optimal one-to-one assignment from it, so that only R slot ids cross PCIe between planning the goals and
 * mnav_fleet_plans.
 *
 * Robots: n of them, given as in mnav_fleet_paths (start_vertex, or start_pos resolved by the rule of mnav_locate with the
 * ids staying on the device).  Columns: slots[0 .. m), DISTINCT plan indices of the recorded Dijkstra call or replan;
 * slots == NULL stands for all its plans in order and m must then equal its plan count.
 * code_out / potential_out: n * m entries, row-major [robot][column].  Entry (i, j) is the code (it fits a byte) and the
 * potential_out that mnav_fleet_paths gives a robot on vertex v_i with slot slots[j], bit for bit, with ONE difference:
 * rule 4 does not walk the chain, it returns MNAV_SUCCESS whenever pred[v] != v.  A chain that does not reach the seed is
 * MNAV_INTERNAL_ERROR in mnav_fleet_paths; here that case is not detected (the pair is MNAV_SUCCESS with potential d[v]).
 * Rule 5 under a finite cut takes the same lazy look at the marked plans as mnav_fleet_paths.
 * A pair is FEASIBLE when its code is MNAV_SUCCESS and its potential is finite; that leaves out every pair of a plan whose
 * seed is its target (rule 2's CAUTION).  nearest_slot_out[i]: the COLUMN INDEX j (not the slot id) of the smallest
 * potential among the feasible pairs of row i, ties to the smallest column, MNAV_NONE for a row without a feasible pair;
 * nearest_robot_out[j]: the same per column, ties to the smallest robot.  vertex_out: as in mnav_fleet_paths.
 * Any output pointer may be NULL; with all of them NULL nothing of the matrix's size leaves the device.  n = 0 does nothing.
 * Returns 0, or -1 with mnav_last_error set and NOTHING touched (no output, no statistic): every refusal of
 * mnav_fleet_paths, m = 0, a slot out of range or given twice, slots == NULL with m different from the plan count, a
 * matrix of more than the option dispatch_max_mb MiB on the device (5 bytes per pair; default 4096).  The call changes no
 * plan output, no layer and no statistic of another entry point; with positions it builds the lookup index of
 * mnav_locate when none exists yet. */
int mnav_fleet_costs(mnav_ctx* ctx, uint32_t n, const uint32_t* start_vertex, const float* start_pos, uint32_t m,
                     const uint32_t* slots, uint8_t* code_out, float* potential_out, uint32_t* vertex_out,
                     uint32_t* nearest_slot_out, uint32_t* nearest_robot_out);
/* The optimal assignment over the matrix of mnav_fleet_costs, which the call computes itself (same robots, columns and
 * refusals; 9 bytes per pair against dispatch_max_mb): a matrix can never be stale.
 * With q_ij = (int64) floor((double) potential_ij / quantum + 0.5) over the feasible pairs, an assignment maps robots to
 * distinct columns over feasible pairs only; the result has MAXIMUM SIZE and, among those, MINIMUM sum of q.  Both numbers
 * are unique; the assignment itself is the one the fixed algorithm below gives, the same in every call.
 * slot_of_robot_out[i] (n): the plan slot id slots[j] of robot i's column -- what mnav_fleet_plans takes -- or MNAV_NONE
 * for a robot without one; robot_of_slot_out[j] (m, per column): its robot or MNAV_NONE; potential_out[i] (n): the pair's
 * float potential, +inf when unassigned; *assigned_out: the size; *total_q_out: the sum of q; *total_potential_out: the
 * double sum of the assigned potentials in robot order.  Any output pointer may be NULL.
 * Algorithm: pad to a square of N = max(n, m); cost q for a feasible pair, M = N q_max + 1 for an infeasible real pair, 0
 * for a pair with a dummy row or column, all multiplied by N + 1; a synchronous (Jacobi) auction in int64 with eps-scaling:
 * eps starts at max(1, C / 2) with C the largest scaled cost and is divided by 8 per phase down to 1, prices are kept
 * across phases and every phase starts with nobody assigned.  In a round every unassigned bidder bids on its best column
 * (smallest cost + price, ties to the smallest column) the column's price + (second-best value - best value) + eps, and
 * every column takes its highest bid (ties to the smallest bidder) and evicts its owner.  A robot left on an M pair or on
 * a dummy column is unassigned.  Rounds with at most dispatch_tail_bidders unassigned bidders (default 16) run inside one
 * single-workgroup kernel, the others as wide launches; the result does not depend on that option.
 * Returns 0, or -1 with mnav_last_error set and NOTHING written: every refusal of mnav_fleet_costs, a quantum that is not
 * finite and positive, a q above 2^31 - 1, (N + 1) (N q_max + 1) >= 2^56 ("quantum too fine for this fleet"), a bid that
 * reaches 2^62, or more than dispatch_max_rounds rounds (default 4194304): the call never hangs. */
int mnav_fleet_assign(mnav_ctx* ctx, uint32_t n, const uint32_t* start_vertex, const float* start_pos, uint32_t m,
                      const uint32_t* slots, double quantum, uint32_t* slot_of_robot_out, uint32_t* robot_of_slot_out,
                      float* potential_out, uint32_t* assigned_out, int64_t* total_q_out, double* total_potential_out);
/* The last mnav_fleet_costs or mnav_fleet_assign that returned 0: pairs[4] = pairs per outcome (MNAV_SUCCESS, beyond the
 * field, without a path, every other code), the feasible pairs; of an assignment (0 after a costs call) its size, phases,
 * rounds, the rounds the tail kernel took and the bids placed; built_index = 1 if the call built the lookup index; device
 * milliseconds of the matrix pass and of the assignment (quantisation to result), host milliseconds of the whole call.
 * Any pointer may be NULL. */
int mnav_dispatch_stats(const mnav_ctx* ctx, uint64_t* pairs, uint64_t* feasible, uint32_t* assigned, uint32_t* phases,
                        uint64_t* rounds, uint64_t* tail_rounds, uint64_t* bids, uint32_t* built_index, float* ms_costs,
                        float* ms_assign, float* ms_total);

/* -- fleet traffic: how many planned paths cross each vertex, and the congestion cost of the excess ------
 * Every fleet call above gives a robot the shortest path of its field as if it were alone.  The calls below close the
 * loop of negotiated congestion on the device: count the paths per vertex, turn the excess into a cost layer, let the
 * layer graph propagate it and replan.  No path id and no V-sized array crosses PCIe.
 *
 * The context owns V uint32 counts c and T, the 64-bit total of the accumulated weight; both are zero after
 * mnav_upload_mesh.  mnav_fleet_traffic takes robots, slots, start_vertex / start_pos, code_out, vertex_out and
 * potential_out exactly as mnav_fleet_paths does and gives them the same values for the same inputs (the lazy look of
 * rule 5 included).  weights[i] (NULL: 1) is the weight w_i of robot i.
 * Robot i CONTRIBUTES iff mnav_fleet_paths gives it MNAV_SUCCESS with a finite potential_out: rule 3 (it stands on the
 * seed) and rule 4 with a chain that reaches the seed; never the seed == target plans of rule 2's CAUTION, no other code.
 * A contributing robot adds w_i to c[v_i] and to c[u] for every id u of its path (pred[v], pred[pred[v]], ..., seed):
 * len + 1 adds, one add -- to c[seed] -- under rule 3; w_i == 0 is classified and adds nothing.  T grows by the weights of
 * the contributing robots.  A path visits a vertex at most once, so no count exceeds T.
 * accumulate == 0: c and T are zeroed first, but only after every refusal check has passed (n = 0 then only zeroes them);
 * accumulate != 0: the call adds on top -- two calls over two halves of a fleet equal one call over the whole fleet; n = 0
 * does nothing.  Sums of integers do not depend on their order: c is the same bits in every call and on every path.
 * Returns 0, or -1 with mnav_last_error set and NOTHING touched (c, T, the outputs and the statistics included): every
 * refusal of mnav_fleet_paths, a field made stale by a cost-changing call included, and the sum of w_i over ALL n robots
 * (as uint64, plus T when accumulating) above 2^32 - 1: "total weight does not fit the counters".  The call changes no plan
 * output, no layer and no statistic of another entry point (mnav_fleet_stats keeps its values); with positions it builds
 * the lookup index of mnav_locate when none exists yet.  Option traffic_combine (default 0): a wave whose contributors all
 * end on one vertex issues one add for them; the counts do not depend on it. */
int mnav_fleet_traffic(mnav_ctx* ctx, uint32_t n, const uint32_t* slots, const uint32_t* start_vertex, const float* start_pos,
                       const uint32_t* weights, int accumulate, uint32_t* code_out, uint32_t* vertex_out, float* potential_out);
/* The counts: V words.  All zero when no traffic call ran since mnav_upload_mesh.  -1: no mesh, a null array. */
int mnav_traffic_download(const mnav_ctx* ctx, uint32_t* counts_out);
/* The last mnav_fleet_traffic that returned 0: robots that contributed with a weight above 0, vertex adds performed, T,
 * the vertices with c > 0 and the largest count after the call; built_index = 1 if the call built the lookup index; device
 * milliseconds of its kernels and host milliseconds of the whole call.  Any pointer may be NULL. */
int mnav_traffic_stats(const mnav_ctx* ctx, uint32_t* contributing, uint64_t* adds, uint64_t* total_weight, uint32_t* occupied,
                       uint32_t* peak, uint32_t* built_index, float* ms_kernels, float* ms_total);
/* The traffic layer, a layer writer like mnav_layer_border.  Per vertex: e = c[v] > free_count ? c[v] - free_count : 0;
 * cost = 0.0f when e == 0, else fminf((float) e * (float) gain, (float) cap) -- conversions round to nearest, one float
 * multiply, no contraction.  No vertex is lethal: traffic is a soft cost.  gain must be finite and >= 0, cap >= 0 and not
 * NaN (+inf: no cap).  changed_out (room for V ids, may be NULL) receives the ascending ids whose cost bits (or lethal
 * flag) differ from what the slot held, for a fresh slot every vertex; *n_changed their number.  The call reads c as it
 * stands and does not care whether the fields are stale.  Returns -1 with mnav_last_error set and the slot untouched on
 * an argument error (no mesh, gain, cap, layer >= 64). */
int mnav_layer_traffic(mnav_ctx* ctx, uint32_t layer, uint32_t free_count, double gain, double cap, uint32_t* changed_out,
                       uint32_t* n_changed);
/* mnav_layer_traffic on an INPUT node of the layer graph, then the propagation, as mnav_map_obstacle does for the obstacle
 * writer: the layer's change list stays on the device, dependents, vertex costs and edge weights follow, changed_out /
 * n_changed receive D as in the other update calls, and the replans' change log receives it -- mnav_fleet_paths and
 * mnav_fleet_traffic refuse the now stale fields until a replan has run.  Refusals: those of the update calls (no computed
 * graph, the layer is not an input node) and the argument errors above; the graph stays usable after them. */
int mnav_map_traffic(mnav_ctx* ctx, uint32_t layer, uint32_t free_count, double gain, double cap, uint32_t* changed_out,
                     uint32_t* n_changed);

/* -- timed fleet traffic: occupancy per (vertex, time window), who holds a cell and who yields --------------
 * mnav_fleet_traffic has no notion of time: two robots that use a corridor ten minutes apart raise its count as two that
 * meet in it.  A field stores dist[u] for every vertex of a robot's chain, so dist[v] - dist[u] is how far along its path
 * the robot is when it reaches u.  The calls below count per (vertex, window), price the PEAK simultaneous use of a vertex
 * and tell every robot where it meets an over-full cell and whether it has to yield; a caller
 * staggers departures (depart[i] += tau for the robots that yield) or prices the peaks and replans.  No path id, no
 * potential and no V-sized array crosses PCIe.
 *
 * The context owns V x windows uint32 cells and V x windows uint32 holders (row-major: cell[v * windows + k]), their own
 * 64-bit total T of the accumulated weight (mnav_fleet_traffic's c, T and statistics are not touched), and per vertex
 * peak[v] = max_k cell[v][k] and peak_window[v] = the smallest k that attains it (MNAV_NONE when the peak is 0).  After
 * mnav_upload_mesh the cells are gone: peaks 0, windows MNAV_NONE, T 0.
 * A call carries `windows` = B windows (1 .. 1024) of width tau (used as (float) tau, finite and > 0); the horizon is
 * B tau.  Robots, slots, start_vertex / start_pos, weights, code_out, vertex_out, potential_out are exactly those of
 * mnav_fleet_traffic (stale fields, the lazy look of rule 5 and the 2^32 - 1 total-weight check included).  Per robot,
 * each may be NULL: depart[i] (NULL: 0; finite and >= 0), pace[i] (NULL: 1; finite and > 0: time per unit of potential --
 * with edge_cost_factor 0 the potential is metres and pace = 1 / speed), key[i] (NULL: i; the priority, smaller wins).
 * Robot i CONTRIBUTES iff mnav_fleet_traffic's rule holds and w_i > 0.  A contributor on vertex v with potential P
 * visits u = v, pred[v], pred[pred[v]], ..., seed: len + 1 visits, one for a robot on the seed.  The window of a visit, all
 * float32, separate operations, no contraction, correctly rounded division:
 *   dt = fmaxf(P - dist[u], 0.f);  t = depart_i + dt * pace_i;  q = t / (float) tau;
 *   in the horizon iff q < (float) B (false for +inf);  k = (uint32_t) q
 * An in-horizon visit adds w_i to cell[u][k] and lowers holder[u][k] (initially 0xFFFFFFFF) to min(holder, key_i); a visit
 * beyond the horizon adds nothing and is counted in the statistics.  T grows by the contributors' weights.  Integer sums
 * and minima do not depend on their order: cells and holders are the same bits in every call, on every schedule, in one
 * call or in several.  A visit at t >= B tau is dropped, never wrapped into an earlier window: windows do not
 * alias.
 * accumulate == 0: cells, holders and T start over -- only after every refusal check has passed; a new (windows, tau)
 * reallocates.  accumulate != 0: the call adds on top of the last one (n = 0 does nothing); a windows or (float) tau other
 * than the cells' is refused.
 * The report is computed after ALL adds of the call, on the cells as they then stand (earlier accumulated calls included).
 * For each contributor, over its in-horizon visits from v to the seed: a visit is OVER when cell[u][k] > free_count; it
 * YIELDS when it is over and holder[u][k] != key_i.  conflict_hops_out[i] = the over visits, yield_hops_out[i] = the
 * yielding visits, first_yield_vertex_out / _window_out / _time_out[i] = u, k and the float t of the first yielding visit
 * in that order; every other robot, and a contributor without a yielding visit: 0 / 0 / MNAV_NONE / MNAV_NONE / +inf.  Robots
 * with EQUAL keys in one cell are both its holders: neither yields there.  With free_count > 0 every robot of an over cell
 * but its holder yields -- more than strictly must, free_count of them could stay; a stagger loop still converges because
 * each round counts again.  Any output may be NULL.
 * Returns 0, or -1 with mnav_last_error set and NOTHING touched (cells, holders, T, outputs and statistics included):
 * everything mnav_fleet_traffic refuses; windows outside 1 .. 1024; a tau that is not finite and positive as a float; a
 * depart that is not finite or is negative; a pace that is not finite or is <= 0 (both checked on the host over all n robots
 * before the first device call); the configuration mismatch under accumulate; 8 V windows bytes above the option
 * timed_traffic_max_mb MiB (default 2048).  mnav_fleet_stats and mnav_traffic_stats keep their values. */
int mnav_fleet_timed_traffic(mnav_ctx* ctx, uint32_t n, const uint32_t* slots, const uint32_t* start_vertex, const float* start_pos,
                             const uint32_t* weights, const float* depart, const float* pace, const uint32_t* key, uint32_t windows,
                             double tau, uint32_t free_count, int accumulate, uint32_t* code_out, uint32_t* vertex_out,
                             float* potential_out, uint32_t* conflict_hops_out, uint32_t* yield_hops_out,
                             uint32_t* first_yield_vertex_out, uint32_t* first_yield_window_out, float* first_yield_time_out);
/* peak_out and window_out: V words each; cells_out and holders_out: V x windows words each, row-major, windows = that of
 * the last call (mnav_timed_traffic_stats).  Any may be NULL.  No timed call since mnav_upload_mesh: peaks 0, windows
 * MNAV_NONE, and there are no cells (nothing is written to cells_out / holders_out).  -1: no mesh. */
int mnav_timed_traffic_download(const mnav_ctx* ctx, uint32_t* peak_out, uint32_t* window_out, uint32_t* cells_out,
                                uint32_t* holders_out);
/* The last mnav_fleet_timed_traffic that returned 0: contributing robots, in-horizon adds, visits beyond the horizon, T;
 * after the call the cells above 0, the cells above its free_count and the largest cell; the robots with yield_hops > 0;
 * its windows; built_index = 1 if the call built the lookup index; device milliseconds of its kernels and host milliseconds
 * of the whole call.  Any pointer may be NULL. */
int mnav_timed_traffic_stats(const mnav_ctx* ctx, uint32_t* contributing, uint64_t* adds, uint64_t* beyond_horizon,
                             uint64_t* total_weight, uint64_t* occupied_cells, uint64_t* over_cells, uint32_t* largest_cell,
                             uint32_t* yielding, uint32_t* windows, uint32_t* built_index, float* ms_kernels, float* ms_total);
/* mnav_layer_traffic's rule on the peaks: cost = traffic cost of (peak[v], free_count, gain, cap), never lethal; the same
 * arguments, change list and argument checks.  It reads the peaks as they stand (all zero before the first timed call). */
int mnav_layer_timed_traffic(mnav_ctx* ctx, uint32_t layer, uint32_t free_count, double gain, double cap, uint32_t* changed_out,
                             uint32_t* n_changed);
/* mnav_layer_timed_traffic on an INPUT node of the layer graph, then the propagation: to it what mnav_map_traffic is to
 * mnav_layer_traffic (the list stays on the device, the replans' change log is written, the same refusals). */
int mnav_map_timed_traffic(mnav_ctx* ctx, uint32_t layer, uint32_t free_count, double gain, double cap, uint32_t* changed_out,
                           uint32_t* n_changed);

/* -- fleet schedule: a departure delay per robot such that no (vertex, window) cell is over capacity -----
 * mnav_fleet_timed_traffic diagnoses: it counts, names a holder and tells every robot whether it yields.  This call is the
 * cure: given the same robots, windows and a capacity it returns a delay per robot, in whole
 * windows, such that no constrained cell exceeds `capacity`, and names the robots that cannot be fitted into the horizon.
 * Robots, slots, start_vertex / start_pos, weights, depart, pace, key, windows = B, tau, accumulate, code_out, vertex_out,
 * potential_out, the defaults, the contributor rule and the float32 window arithmetic are exactly those of
 * mnav_fleet_timed_traffic.  capacity >= 1 plays the role free_count plays in the report; max_delay (0 .. B - 1) is in
 * whole windows; max_rounds = 0 means no limit; flags: MNAV_SCHEDULE_SEED_FREE or 0.
 * A contributor i tries delay d with depart_d = depart_i + (float) d * (float) tau (one multiply, then one add, no
 * contraction: d = 0 gives depart_i bit for bit).  Its visits then fall at t = depart_d + fmaxf(P - dist[u], 0) * pace_i
 * into the window of t.  Candidate d FITS iff every visit lies inside the horizon -- a schedule does not commit a robot to a
 * trip it cannot see the end of -- and every CONSTRAINED visit has cell[u][k] + w_i <= capacity.  Every visit is
 * constrained; with MNAV_SCHEDULE_SEED_FREE the last one, on the seed, is not (arrivals at a goal or depot are not
 * rationed, but they are still counted on commit).  A robot with w_i > capacity never fits.
 * Rounds r = 1, 2, ... on the committed cells and a current delay cur per robot (0 at the start):
 *   probe   every OPEN robot takes the smallest d in [cur, max_delay] that fits the cells as they stand at the start of
 *           the round and sets cur = d; none fits: MNAV_SCHEDULE_NO_SLOT, for good (cells only grow)
 *   claim   every robot that found a d adds w_i to a tentative count of each constrained visit's cell and lowers the cell's
 *           tentative holder to (key_i, i), ordered lexicographically: equal keys are broken by the smaller index
 *   decide  a robot WINS iff for every constrained visit cell + tentative <= capacity or the tentative holder is the robot
 *   commit  every winner is MNAV_SCHEDULE_COMMITTED with delay d in round r: ALL its visits (the seed's too) add w_i to
 *           cell[u][k] and lower holder[u][k] to key_i, T grows by w_i; losers stay OPEN and probe again from cur
 * until nobody is OPEN or r == max_rounds (robots still OPEN then report MNAV_SCHEDULE_OPEN).  With flags = 0 and
 * accumulate = 0 no cell exceeds capacity; every round with an OPEN robot that found a delay commits at least the one with
 * the smallest (key, index), so the loop ends within n rounds; sums and minima of integers do not depend on their order, so
 * outputs and cells are the same bits on every run, with any schedule_chunk_rounds and either schedule_clean_fill.
 * NOT claimed: the result is not the sequential "robots in key order" greedy schedule -- the rule above is its own
 * definition; and two accumulating calls over two halves of a fleet are not one call over the whole fleet, unlike counting.
 * The cells ARE the timed cells: the call writes the context's cells, holders, T, windows and tau and ends with the peak
 * pass at free_count = capacity, so mnav_timed_traffic_download, mnav_layer_timed_traffic and mnav_map_timed_traffic see the
 * schedule.  accumulate has mnav_fleet_timed_traffic's meaning: existing cells count as reservations, whoever made them
 * (robots under way counted by a timed call, or an earlier schedule); cells already above capacity are simply blocked.
 * mnav_timed_traffic_stats afterwards describes the cells as if the committed robots had been a timed call's
 * contributors: contributing = the committed robots, adds = their visits, beyond_horizon = 0, yielding = 0, total_weight =
 * T, occupied / over (above capacity) / largest from the peak pass, windows = B.
 * Per robot, each may be NULL: status_out (MNAV_SCHEDULE_NONE for a robot that does not contribute); delay_out and
 * round_out (MNAV_NONE unless committed); depart_out = depart_d of the committed delay, else +inf.
 * Returns 0, or -1 with mnav_last_error set and NOTHING touched (cells, outputs, statistics): everything
 * mnav_fleet_timed_traffic refuses; capacity == 0; max_delay >= windows; an unknown flag bit; 20 V windows bytes (cells,
 * holders and the call's tentative arrays) above the option timed_traffic_max_mb.  n = 0 behaves as in the timed call.
 * mnav_fleet_stats and mnav_traffic_stats keep their values. */
#define MNAV_SCHEDULE_NONE 0u
#define MNAV_SCHEDULE_COMMITTED 1u
#define MNAV_SCHEDULE_NO_SLOT 2u
#define MNAV_SCHEDULE_OPEN 3u
#define MNAV_SCHEDULE_SEED_FREE 1u
int mnav_fleet_schedule(mnav_ctx* ctx, uint32_t n, const uint32_t* slots, const uint32_t* start_vertex, const float* start_pos,
                        const uint32_t* weights, const float* depart, const float* pace, const uint32_t* key, uint32_t windows,
                        double tau, uint32_t capacity, uint32_t max_delay, uint32_t max_rounds, uint32_t flags, int accumulate,
                        uint32_t* code_out, uint32_t* vertex_out, float* potential_out, uint32_t* status_out, uint32_t* delay_out,
                        float* depart_out, uint32_t* round_out);
/* The last mnav_fleet_schedule that returned 0: contributing, committed, NO_SLOT and still OPEN robots; the rounds that ran;
 * the committed robots with a delay above 0 and the largest committed delay; claims = the sum over the rounds of the robots
 * that claimed; the visits of the committed robots; built_index = 1 if the call built the lookup index; device milliseconds
 * of its kernels and host milliseconds of the whole call.  Any pointer may be NULL. */
int mnav_schedule_stats(const mnav_ctx* ctx, uint32_t* contributing, uint32_t* committed, uint32_t* no_slot, uint32_t* open,
                        uint32_t* rounds, uint32_t* delayed, uint32_t* max_delay_used, uint64_t* claims, uint64_t* committed_visits,
                        uint32_t* built_index, float* ms_kernels, float* ms_total);

/* -- one plan over several GPUs (BASELINE config 4) ---------------------------------------------
 * The reference's loop (dijkstra_mesh_planner.cpp:287-348) on a mesh that is range-partitioned over `world`
 * processes, one per GPU: the LDS tiles are in Morton order and process `rank` owns a contiguous range of them.
 * Every process uploads the same mesh and costs, then
 *   n = mnav_shard_setup(ctx, rank, world)            floats in the exchange buffer (interface vertices + robot vertex)
 *   mnav_shard_begin(ctx, seed, target, offset, limit)
 *   repeat { mnav_shard_rounds(ctx, R, buf);           R local tile rounds, then buf[i] = own interface values / +inf
 *            min-allreduce(buf) over the processes      (RCCL over xGMI; ncclAllReduce(ncclMin) / torch.distributed)
 *            mnav_shard_apply(ctx, buf, &local_min, &target_dist);
 *          } until min-allreduce(local_min) is +inf or > target_dist + offset
 *   mnav_shard_finalize(ctx, dist_buf, pred_buf);       owned entries, +inf / 0xFFFFFFFF elsewhere: min-allreduce both
 * `buf`, `dist_buf` (V floats) and `pred_buf` (V uint32) are DEVICE pointers owned by the caller (the collective runs on
 * them in place).  The result is bit-identical to the single-GPU plan: the schedule is label-correcting, only the
 * fixed point matters.  Returns 0, <0 on error, 1 if cancelled. */
int mnav_shard_setup(mnav_ctx* ctx, uint32_t rank, uint32_t world);
int mnav_shard_info(const mnav_ctx* ctx, uint32_t* t_lo, uint32_t* t_hi, uint32_t* ntiles, uint32_t* n_exchange);
/* The same loop on a mesh whose DATA is partitioned (north_star: "the mesh is range-partitioned across the 8 GPUs ...
 * allreduce of halo-vertex distances only"): the mesh uploaded to this context is ONE PART -- the vertices this process
 * owns plus their 1-ring halo (the neighbours owned elsewhere), renumbered in ascending global id, with every edge that has
 * an owned endpoint.  `exchange_vertex[i]` (i < n_exchange, the same global list of interface vertices on every process:
 * the vertices that have a neighbour owned by another process) is the LOCAL id of interface vertex i, or 0xFFFFFFFF when
 * this process does not hold it; `owned[v]` (one byte per local vertex) is 1 for owned vertices, 0 for halo copies.
 * The exchange buffer has n_exchange + 1 floats (last: the robot vertex, passed to mnav_shard_begin as a local id).  All
 * local tiles run; every held copy of an interface vertex is packed (a value reached along real edges is an upper bound of
 * the true distance) and takes the reduced minimum; mnav_shard_finalize returns dist / pred of the LOCAL vertices (the
 * owned ones are final, predecessors are local ids), sized by the part, not by the mesh.  Returns n_exchange + 1. */
int mnav_shard_setup_partition(mnav_ctx* ctx, uint32_t n_exchange, const uint32_t* exchange_vertex, const uint8_t* owned);
/* After mnav_shard_finalize: one segment of the vertex path (dijkstra_mesh_planner.cpp:358-373) inside this process's part.
 * Predecessors are followed from `start_vertex` (local id) while the vertex is owned here, at most `cap` hops:
 * out_host[0] = hops, out_host[1] = the vertex the walk stopped at (the seed, or a halo copy: its owner continues),
 * out_host[2] = 1 if a vertex without predecessor was met (the wave never reached it), out_host[3..] = the predecessors
 * visited (local ids).  `out_host` holds cap + 3 words.  The potential / predecessor arrays never leave the device. */
int mnav_shard_walk(mnav_ctx* ctx, uint32_t start_vertex, uint32_t seed_vertex, uint32_t cap, uint32_t* out_host);
/* Device memory this context holds for mesh tables and per-plan state, in bytes (the partitioned plan's footprint test). */
uint64_t mnav_device_bytes(const mnav_ctx* ctx);

int mnav_shard_begin(mnav_ctx* ctx, uint32_t seed_vertex, uint32_t target_vertex, double goal_dist_offset, double cost_limit);
/* Partitioned data, negative goal_dist_offset only: with such an offset the reference expands exactly the vertices popped BEFORE
 * the robot vertex (dijkstra_mesh_planner.cpp:293-300), and among vertices of the robot vertex's potential the vertex id decides.
 * A part that does not hold the robot vertex passes the robot's RANK among its own (ascending) ids -- the number of local vertices
 * with a smaller global id -- before mnav_shard_begin; parts that hold it need not call this. */
int mnav_shard_set_goal_tie(mnav_ctx* ctx, uint32_t tie_id);
int mnav_shard_rounds(mnav_ctx* ctx, uint32_t rounds, float* iface_buf_dev);
int mnav_shard_apply(mnav_ctx* ctx, const float* iface_buf_dev, float* local_min_out, float* target_dist_out);
int mnav_shard_finalize(mnav_ctx* ctx, float* dist_buf_dev, uint32_t* pred_buf_dev);
/* The two steps of an exchange without a host round trip.  `caller_stream` (a hipStream_t) is the stream the caller's
 * collectives are ordered on; the library links its own stream to it with events in both directions, nothing waits on the
 * host.  mnav_shard_apply_async writes {smallest pending wake-up, dist[target], -1 if mnav_cancel arrived else 0} to the
 * DEVICE words ctl_dev[0..2]; the caller min-allreduces them and reads them back once every few exchanges -- an exchange
 * after convergence changes nothing, so checking late is safe. */
int mnav_shard_rounds_async(mnav_ctx* ctx, uint32_t rounds, float* iface_buf_dev, void* caller_stream);
int mnav_shard_apply_async(mnav_ctx* ctx, const float* iface_buf_dev, float* ctl_dev, void* caller_stream);

/* Replaces MeshPlanner::cancel(), mesh_planner.h:80 (dijkstra_mesh_planner.cpp:136-140):
 * async-signal/thread safe, only sets a flag that the running plan polls between step
 * batches; the plan then returns MNAV_CANCELED.  The flag is cleared when a plan starts
 * (dijkstra_mesh_planner.cpp:238). */
void mnav_cancel(mnav_ctx* ctx);

/* -- introspection / tuning -------------------------------------------------------------- */
int mnav_get_stats(const mnav_ctx* ctx, mnav_stats* out);
/* The same without the settled-vertex count when that has not been taken yet: after a paths-only batch of the tile-batch
 * engine the count (instrumentation for mnav_algorithmic_bytes) is made by the first mnav_get_stats / mnav_algorithmic_bytes
 * call, from the resident distances -- mnav_get_timing never triggers it and reports settled = 0 until then. */
int mnav_get_timing(const mnav_ctx* ctx, mnav_stats* out);
/* What the finalize pass of the last tile-batch call kept from the call before it and left for the next one (option
 * tb_fin_keep).  skipped_pairs: (tile, plan) pairs whose dist / pred / vecmap stores it left out, because the plan's wave did
 * not come near the tile and the slot's arrays held that pattern from the previous pass already; reset_pairs: pairs whose
 * slice of the distance buffer it reset to +inf itself (0: the buffer is cleaned by a fill); filled_at_start: 1 when the call
 * had to fill the distance buffer before it could start.  The pairs are counted on this call, from the maps the pass left; all
 * three are 0 after a call that ran no finalize pass except filled_at_start.  Returns 0, or -1 (mnav_last_error). */
int mnav_tb_finalize_stats(mnav_ctx* ctx, uint64_t* skipped_pairs, uint64_t* reset_pairs, uint32_t* filled_at_start);
/* The counters of the last run of the tile-batch engine (all 0 before the first): iterations of the engine; work items (one tile
 * with up to 64 plans of its bucket under k_tbv_solve, up to 16 under k_tb_solve_q); activations ((tile, plan) pairs solved);
 * Gauss-Seidel sweeps, one per item and sweep -- sweeps / items is what the option tb_sweep_seq lowers; (tile, plan) pairs woken.
 * Concurrent waves see each other's exports sooner or later, so iterations, items and activations of the same batch differ from
 * run to run; the results never do.  Any pointer may be null.  Returns 0, or -1 without a context. */
int mnav_tb_engine_stats(const mnav_ctx* ctx, uint32_t* iterations, uint64_t* items, uint64_t* activations, uint64_t* sweeps, uint64_t* wakes);
/* Band width of the wavefront engine in potential units; <= 0 selects the default
 * (3 x mean finite edge weight for the Dijkstra band steps, 12 x for CVP, recomputed on every cost
 * upload).  Results do not depend on it. */
int mnav_set_band_width(mnav_ctx* ctx, float delta);
/* Schedule of the Dijkstra planner: 0 = LDS-tiled label-correcting rounds (one launch per round),
 * 1 = the distance-band gather steps that the CVP planner uses,
 * (2, one persistent workgroup per plan, was retired in round 5: -1),
 * 3 = automatic (default): 6 for calls of up to `async_max_batch` = 160 plans (a call whose ticket ring overflows is re-run on 0),
 *     5 beyond that (batches that also hold >= tiles/1000 plans), else 0,
 * 5 = tile-batch: one plan per lane, the tile's graph as record streams (highest throughput for large batches); its tiles are
 *     solved by k_tbv_solve (one wave per tile, <= 64 plans, the distances in VGPRs) when a tile sees enough plans per iteration
 *     (plans / sqrt(tiles) >= 8, option "tb_kernel" overrides), else by k_tb_solve_q (16 plans per quarter of a wave, LDS),
 * 6 = the LDS tiles without rounds: resident workgroups serve a ticket queue of woken tiles, solve and wake tiles
 *     asynchronously, one launch per call (single plans -- what MeshPlanner::makePlan runs -- and batches up to ~100 plans).
 * All give identical results (the label-correcting fixed point does not depend on the schedule). */
int mnav_set_dijkstra_engine(mnav_ctx* ctx, int engine);
/* Tuning / debug options by name (the list with one line each: mesh_navigation_amd/csrc/mnav_options.h; e.g. "cvp_wide",
 * "cvp_groups", "no_graph", "lazy_paths", "max_wall_s", "async_wg_per_plan").  mnav_create reads the process environment ONCE
 * (MNAV_<NAME>); afterwards this call is the only way to change an option -- no plan path ever looks at the environment.
 * value = NaN restores the built-in default.  Options read at upload time ("tile_size", "tb_tile") act on the next
 * mnav_upload_mesh.  Returns 0, or -1 for an unknown name; mnav_get_option returns NaN for unset / unknown. */
int mnav_set_option(mnav_ctx* ctx, const char* name, double value);
double mnav_get_option(const mnav_ctx* ctx, const char* name);
/* Outputs that stay on the device.  mnav_set_resident_outputs(ctx, 1): every plan also computes its vector map
 * (computeVectorMap, dijkstra :189-209 / cvp :204-239) and leaves it in HBM even when no host buffer is passed.
 * mnav_download_output copies one V-sized output of plan `slot` to the host on demand (what as below; 12 B/vertex for
 * the vector map, 4 B otherwise).  mnav_vector_at is MeshMap::directionAtPosition (mesh_map.cpp:625-650) on the
 * resident vector map: the controller's sample at the robot pose (returns 1, 0 = no vector there, <0 error). */
int mnav_set_resident_outputs(mnav_ctx* ctx, int on);
int mnav_download_output(mnav_ctx* ctx, uint32_t slot, int what, void* host_out);
int mnav_vector_at(mnav_ctx* ctx, uint32_t slot, const uint32_t vs[3], const float bary[3], float out[3]);
/* CVPMeshPlanner's back-tracking over the vector field (cvp_mesh_planner.cpp:920-951: MeshMap::meshAhead mesh_map.cpp
 * :1070-1108 with projectedBarycentricCoords util.cpp:320-347, searchNeighbourFaces mesh_map.cpp:999-1068,
 * directionAtPosition :625-650 and InflationLayer::vectorAt inflation_layer.cpp:493-521) on the vector maps the last
 * mnav_plan_cvp(_batch) call left resident (mnav_set_resident_outputs, or a vecmap_out buffer): plan i walks from
 * target_pos/target_face (the robot) until it is within step_width of seed_pos/seed_face (the goal).  inflation_layer: a
 * layer computed by mnav_layer_inflation whose repulsive field is added to every step, or -1.  Row i of positions_out
 * (cap*3 floats) / faces_out (cap) receives n_out[i] entries in the reference's list order (seed first); status_out[i] =
 * 1 reached the seed, 0 no path (the walk left the field or the mesh, or ran into `cap`), -1 a face of the walk has a
 * vertex without an inflation entry (lvr2 panics there), -2 internal list overflow.  The same float32 operations in the
 * same order as the host: positions are bit-identical.  Returns 0, or -1 with mnav_last_error set (then nothing was
 * walked).  The single-plan form returns the status; -1 with a non-empty mnav_last_error is an argument/device error. */
int mnav_backtrack_cvp_batch(mnav_ctx* ctx, uint32_t n, const float* seed_pos, const uint32_t* seed_faces, const float* target_pos,
                             const uint32_t* target_faces, double step_width, int32_t inflation_layer, uint32_t cap,
                             float* positions_out, uint32_t* faces_out, uint32_t* n_out, int32_t* status_out);
int mnav_backtrack_cvp(mnav_ctx* ctx, const float seed_pos[3], uint32_t seed_face, const float target_pos[3], uint32_t target_face,
                       double step_width, int32_t inflation_layer, uint32_t cap, float* positions_out, uint32_t* faces_out,
                       uint32_t* n_out);
/* Device pointers of the last plan's resident outputs (slot = plan index in a batch):
 * what = 0 dist, 1 pred, 2 direction, 3 cutface, 4 vecmap.  NULL if not available -- in particular dist / pred after a
 * paths-only Dijkstra call (no dist_out / pred_out / vector map asked for): such a call runs no finalize pass, values
 * beyond goal_dist would be engine-tentative.  mnav_download_output additionally takes what = 5, the POPPED potential of
 * a Dijkstra plan: the reference's value wherever it popped the vertex (dist <= goal_dist), +inf elsewhere.
 * After a new mnav_upload_mesh and until the next plan call every output of the old mesh is gone: mnav_device_output
 * returns NULL and mnav_download_output returns -1 with "output not resident", for what = 5 as for the others, before
 * anything is allocated or launched. */
const void* mnav_device_output(const mnav_ctx* ctx, uint32_t slot, int what);
/* Algorithmic bytes of the last call per SURVEY.md §8(d): SSSP 24*V' + 24*E', CVP 32*V' + 68*F'
 * with V' = settled vertices and E'/F' their incident edges/faces scaled from the full mesh. */
uint64_t mnav_algorithmic_bytes(const mnav_ctx* ctx);
/* Which engine / kernel ran the last Dijkstra call (for reports and profiles): the engine of mnav_set_dijkstra_engine that `auto`
 * resolved to (0, 1, 5, 6), + 16 when the tile-batch engine (5) solved its tiles with the register-resident kernel k_tbv_solve
 * (64 plans per wave, distances in VGPRs) instead of k_tb_solve_q (16 plans per quarter of a wave, distances in LDS).  -1: none
 * (no Dijkstra call yet, none whose plans reached the device, or a new mnav_upload_mesh since). */
int mnav_last_engine(const mnav_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* MNAV_H */
