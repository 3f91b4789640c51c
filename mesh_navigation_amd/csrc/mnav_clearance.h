// mnav_clearance.h -- the clearance and border layers (mnav_layer_clearance, mnav_layer_border; ClearanceLayer,
// clearance_layer.cpp:67-99 / :122-164, and BorderLayer, border_layer.cpp:66-80 / :104-110, of mesh_layers;
// include/mnav.h).
//
// Clearance: one ray per vertex from p_v along its resident normal, closest hit over the obstacle layer's LBVH
// (mnav_obstacle.h) with the faces that have v as a corner left out; the array is cached on the context and the cost
// pass (computeLethalsAndCosts) runs on every call.  Border: v is a border vertex iff an edge of its CSR row has fewer
// than two incident faces, counted over v's corner table.  Both end in the diff + compaction pass of mnav_changelist.h,
// comparing the cost bits as well as the lethal flag.
//
// The per-vertex rules (self-exclusion, usable normal, border predicate, the two cost mappings) are MNAV_HD functions
// that g++ compiles too (tests/test_clearance_model.py); clr_vertex_host is the brute-force cast of one vertex on the
// host.  The kernels below them are device only.
#pragma once

#include <math.h>
#include <stdint.h>

#include "mnav_eval.h"   // MNAV_HD
#include "mnav_ray.h"

namespace mnav_clr {

constexpr double kPi = 3.14159265358979323846;   // M_PI

// a face with v as a corner is never hit by v's own ray (compared by vertex id, not by position)
MNAV_HD bool clr_excluded(uint32_t v, uint32_t a, uint32_t b, uint32_t c) { return a == v || b == v || c == v; }

// a normal that casts: finite and not the zero vector (otherwise the clearance is +inf)
MNAV_HD bool clr_normal_usable(float nx, float ny, float nz)
{
  return isfinite(nx) && isfinite(ny) && isfinite(nz) && !(nx == 0.f && ny == 0.f && nz == 0.f);
}

// ClearanceLayer::computeLethalsAndCosts (clearance_layer.cpp:77-95) in double, stored as float
MNAV_HD float clr_cost(float clearance, double robot_height, double height_inflation, uint8_t* lethal)
{
  const double c = (double)clearance;
  if (c < robot_height) { *lethal = 1; return 1.0f; }
  *lethal = 0;
  if (c < robot_height + height_inflation) {
    const double diff = (c - robot_height) / height_inflation;
    return (float)((cos(diff * kPi) + 1.0) / 2.0);
  }
  return 0.0f;
}

// BorderLayer: border_cost on border vertices, 0 elsewhere (as float); lethal iff (double)cost > threshold (:66-80)
MNAV_HD float border_cost_of(bool border, double border_cost, double threshold, uint8_t* lethal)
{
  const float cost = border ? (float)border_cost : 0.0f;
  *lethal = (double)cost > threshold ? 1 : 0;
  return cost;
}

// v's CSR row lists the edge ids nbr_e[rb, re); v's corners crn[cb, ce) name the two sides of their face at v (ea =
// (v2, v), eb = (v, v1): mnav_build.h).  v is a border vertex iff one of its edges is used by fewer than two of its
// corners, i.e. has fewer than two incident faces.  A vertex without edges is not a border vertex.
template <class Crn>
MNAV_HD bool border_vertex(const uint32_t* nbr_e, uint32_t rb, uint32_t re, const Crn* crn, uint32_t cb, uint32_t ce)
{
  for (uint32_t k = rb; k < re; ++k) {
    const uint32_t e = nbr_e[k];
    uint32_t n = 0;
    for (uint32_t i = cb; i < ce; ++i) n += (crn[i].ea == e ? 1u : 0u) + (crn[i].eb == e ? 1u : 0u);
    if (n < 2) return true;
  }
  return false;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One vertex on the host, by brute force over all F faces: the clearance the kernel finds over the BVH (closest hit,
// equal t to the smallest face id, +inf without a hit or a usable normal).  `hits` (may be null) gets 1 on a hit.
inline float clr_vertex_host(uint32_t v, const float* xyz, const float* nrm, const uint32_t* faces, uint32_t F, int* hit_out)
{
  if (hit_out) *hit_out = 0;
  const float* n = nrm + 3 * (size_t)v;
  if (!clr_normal_usable(n[0], n[1], n[2])) return INFINITY;
  const mnav::RaySetup s = mnav::ray_setup(n[0], n[1], n[2]);
  const float* o = xyz + 3 * (size_t)v;
  float best = INFINITY;
  uint32_t best_f = 0xFFFFFFFFu;
  for (uint32_t f = 0; f < F; ++f) {
    const uint32_t a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    if (clr_excluded(v, a, b, c)) continue;
    float t;
    if (mnav::ray_triangle(s, o, xyz + 3 * (size_t)a, xyz + 3 * (size_t)b, xyz + 3 * (size_t)c, &t) && (t < best || (t == best && f < best_f))) {
      best = t;
      best_f = f;
    }
  }
  if (hit_out) *hit_out = best_f != 0xFFFFFFFFu;
  return best_f != 0xFFFFFFFFu ? best : INFINITY;
}
#endif

}  // namespace mnav_clr

#if defined(__HIPCC__)
namespace mnav_clr {

// Per-context state: the cached clearance and the border flags; dropped by mnav_upload_mesh.
struct State {
  bool valid = false;            // clr holds the clearance of the resident mesh and normals
  DevBuf<float> clr;             // V
  DevBuf<uint8_t> border;        // V: border flags of the last mnav_layer_border
  uint32_t cast = 0, rays = 0, hits = 0;
  float ms_build = 0.f, ms_cast = 0.f, ms_total = 0.f;
};

struct CastArgs {
  uint32_t V, F, root;
  const float* __restrict__ xyz;
  const float* __restrict__ nrm;
};

// One lane per vertex, in vertex order: the obstacle layer's closest-hit traversal (bvh_closest_hit) with the LDS stack,
// each lane with its own RaySetup and slab inverses; faces with v as a corner are skipped at the leaves (Bvh::fvtx).
__global__ __launch_bounds__(mnav_obs::kCastBlock) void k_clr_cast(CastArgs A, const float4* __restrict__ nodes, const float4* __restrict__ tris,
                                                         const uint32_t* __restrict__ fvtx, float* __restrict__ clr, uint32_t* __restrict__ cnt)
{
  __shared__ uint32_t stack[mnav_obs::kStack * mnav_obs::kCastBlock];
  const uint32_t lane = threadIdx.x;
  const uint32_t v = blockIdx.x * mnav_obs::kCastBlock + lane;
  bool cast = false, hit = false, over = false;
  if (v < A.V) {
    const float n[3] = { A.nrm[3 * (size_t)v], A.nrm[3 * (size_t)v + 1], A.nrm[3 * (size_t)v + 2] };
    float best = INFINITY;
    uint32_t best_f = kNone;
    if (clr_normal_usable(n[0], n[1], n[2]) && A.F) {
      cast = true;
      const float o[3] = { A.xyz[3 * (size_t)v], A.xyz[3 * (size_t)v + 1], A.xyz[3 * (size_t)v + 2] };
      const mnav::RaySetup rs = mnav::ray_setup(n[0], n[1], n[2]);
      float inv[3];
      for (int a = 0; a < 3; ++a) inv[a] = mnav::ray_slab_inverse(n[a]);
      over = mnav_obs::bvh_closest_hit(A.F, A.root, nodes, tris, rs, o, inv, stack, lane,
        [&](uint32_t f) { return clr_excluded(v, fvtx[3 * (size_t)f], fvtx[3 * (size_t)f + 1], fvtx[3 * (size_t)f + 2]); }, &best, &best_f);
      hit = best_f != kNone;
    }
    clr[v] = hit ? best : INFINITY;
  }
  const uint64_t bc = __ballot(cast), bh = __ballot(hit), bo = __ballot(over);
  if (lane == 0) {
    if (bc) atomicAdd(&cnt[mnav_chg::kKept], (uint32_t)__popcll(bc));
    if (bh) atomicAdd(&cnt[mnav_chg::kHits], (uint32_t)__popcll(bh));
    if (bo) atomicAdd(&cnt[mnav_chg::kOverflow], 1u);
  }
}

// One lane per vertex, no atomics: the border predicate over the resident CSR row and corner table.
__global__ __launch_bounds__(256) void k_border(uint32_t V, const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ nbr_e,
                                                const uint32_t* __restrict__ crn_ptr, const CornerIdx* __restrict__ crn, uint8_t* __restrict__ border)
{
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  border[v] = border_vertex(nbr_e, row_ptr[v], row_ptr[v + 1], crn, crn_ptr[v], crn_ptr[v + 1]) ? 1 : 0;
}

// change-list rules: a vertex changed iff its lethal flag or its cost bits did, and every vertex of a fresh slot
struct ClearanceRule {
  static constexpr bool kCostBits = true;
  const float* __restrict__ clr;
  double robot_height, height_inflation;
  __device__ __forceinline__ float operator()(size_t v, uint8_t* lethal) const { return clr_cost(clr[v], robot_height, height_inflation, lethal); }
};

struct BorderRule {
  static constexpr bool kCostBits = true;
  const uint8_t* __restrict__ border;
  double border_cost, threshold;
  __device__ __forceinline__ float operator()(size_t v, uint8_t* lethal) const { return border_cost_of(border[v] != 0, border_cost, threshold, lethal); }
};

}  // namespace mnav_clr
#endif
