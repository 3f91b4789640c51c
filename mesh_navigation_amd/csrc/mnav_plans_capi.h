// mnav_plans_capi.h -- the C ABI of the fleet plans (include/mnav.h: mnav_upload_face_normals, mnav_fleet_plans,
// mnav_fleet_walk_plans) over the kernels of mnav_plans.h and the shared steps of mnav_fleet_capi.h.  Included by mnav.hip
// inside its extern "C" block, after mnav_fleet_capi.h.
#pragma once

int mnav_upload_face_normals(mnav_ctx* ctx, uint32_t F, const float* face_normals)
{
  if (!ctx) return -1;
  ctx->err.clear();
  if (!ctx->have_mesh) { ctx->err = "mnav_upload_mesh has not been called"; return -1; }
  if (F != ctx->F) { ctx->err = "face normals: F differs from the resident mesh"; return -1; }
  if (F && !face_normals) { ctx->err = "face normals: null array"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return -1; }
  ctx->have_face_normals = false;
  HIPCHK(ctx->d_fnrm.upload(ctx->stream, face_normals, 3 * (size_t)F));
  HIPCHK(hipStreamSynchronize(ctx->stream));                          // the caller's array may go out of scope
  ctx->have_face_normals = true;
  return 0;
}

int mnav_fleet_plans(mnav_ctx* ctx, uint32_t n, const uint32_t* slots, const uint32_t* start_vertex, const float* start_pos, uint32_t n_plans,
                     const float* goal_pos, uint32_t* code_out, uint32_t* vertex_out, float* potential_out, uint32_t* len_out, uint64_t* offset_out,
                     double* cost_out, double* poses_out, uint64_t poses_cap, uint64_t* total_out)
{
  using namespace mnav_fleet;
  if (!ctx) return -1;
  ctx->err.clear();
  if (!n) return 0;
  FleetCall R{ ctx, "fleet plans", n, slots, start_vertex, start_pos };
  if (R.begin(!start_pos || !goal_pos ? "null start or goal positions" : nullptr)) return -1;   // (the positions are the poses' ends, with start vertices too)
  if (!ctx->have_normals) { ctx->err = "fleet plans: vertex normals are not resident (mnav_upload_mesh with vertex_normals)"; return -1; }
  if (n_plans != R.fields.size()) { ctx->err = "fleet plans: n_plans differs from the last plan call"; return -1; }
  if (R.classify()) return -1;
  State& S = ctx->fleet;
  PlanState& PS = ctx->plans;
  if (plans_reserve(ctx, n, n_plans, 0, 0)) return -1;
  const float* d_start = S.pos;                                       // the robot positions: the lookup keeps them when it ran
  if (start_vertex) HIPCHK(hipMemcpyAsync(S.pos, start_pos, 12 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  else d_start = ctx->loc.q;
  HIPCHK(hipMemcpyAsync(PS.goal, goal_pos, 12 * (size_t)n_plans, hipMemcpyHostToDevice, ctx->stream));
  const uint32_t nb = (n + kFleetBlock - 1) / kFleetBlock;
  hipLaunchKernelGGL(k_plan_count, dim3(nb), dim3(kFleetBlock), 0, ctx->stream, n, S.len.get(), PS.count.get(), S.bsum.get());   // (the block sums of the hops are not needed)
  hipLaunchKernelGGL(k_fleet_scan, dim3(1), dim3(kFleetBlock), 0, ctx->stream, nb, S.bsum.get(), (const unsigned long long*)nullptr, S.off + n);
  hipLaunchKernelGGL(k_fleet_offsets, dim3(nb), dim3(kFleetBlock), 0, ctx->stream, n, PS.count.get(), S.bsum.get(), S.off.get());
  unsigned long long total = 0; uint32_t cnt[kCounters + 1] = {};
  if (R.finish(&total, cnt)) return -1;
  const bool fits = poses_out && total <= poses_cap;
  if (plans_reserve(ctx, n, n_plans, total, fits ? total : 0)) return -1;
  HIPCHK(hipEventRecord(S.ev[0], ctx->stream));
  if (total) {
    PlanView Q{};
    Q.n = n; Q.V = ctx->V; Q.xyz = ctx->d_xyz.get(); Q.vn = ctx->d_nrm.get(); Q.start = d_start; Q.goal = PS.goal.get(); Q.slot = S.slot.get(); Q.count = PS.count.get();
    Q.ids = PS.ids.get(); Q.off = S.off.get();
    hipLaunchKernelGGL(k_fleet_write, dim3(nb), dim3(kFleetBlock), 0, ctx->stream, R.P, S.off.get(), PS.ids.get());   // robot i's hops at its pose offset
    hipLaunchKernelGGL(k_plan_poses, dim3((uint32_t)((total + kFleetBlock - 1) / kFleetBlock)), dim3(kFleetBlock), 0, ctx->stream, Q, total,
                       fits ? PS.poses.get() : (double*)nullptr, PS.lengths.get());
  }
  hipLaunchKernelGGL(k_plan_cost, dim3(nb), dim3(kFleetBlock), 0, ctx->stream, n, PS.count.get(), S.off.get(), PS.lengths.get(), PS.cost.get());
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(S.ev[1], ctx->stream));
  if (fits && total) HIPCHK(hipMemcpyAsync(poses_out, PS.poses, sizeof(double) * kPoseDoubles * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));   // one dense copy
  if (R.download(code_out, vertex_out, potential_out)) return -1;
  if (len_out) HIPCHK(hipMemcpyAsync(len_out, PS.count, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (offset_out) HIPCHK(hipMemcpyAsync(offset_out, S.off, 8 * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->stream));
  if (cost_out) HIPCHK(hipMemcpyAsync(cost_out, PS.cost, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  S.stats.ms_kernels += ev_ms(S.ev[0], S.ev[1]);
  if (total_out) *total_out = total;
  R.report(cnt, total);
  return fits ? 0 : 1;
}

int mnav_fleet_walk_plans(mnav_ctx* ctx, uint32_t n, const uint32_t* slots, uint32_t n_plans, const float* seed_pos, const uint32_t* seed_faces,
                          const double* goal_pose, const float* start_pos, const uint32_t* start_faces, double step_width, int32_t inflation_layer,
                          uint32_t walk_cap, int32_t* status_out, uint32_t* start_face_out, uint32_t* len_out, uint64_t* offset_out, double* cost_out,
                          double* poses_out, uint64_t poses_cap, uint64_t* total_out)
{
  return fleet_walks_run(ctx, true, n, slots, n_plans, seed_pos, seed_faces, goal_pose, start_pos, start_faces, step_width, inflation_layer, walk_cap, status_out,
                         start_face_out, len_out, offset_out, nullptr, nullptr, cost_out, poses_out, poses_cap, total_out);
}
