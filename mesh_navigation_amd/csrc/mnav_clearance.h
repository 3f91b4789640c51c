// mnav_clearance.h -- the clearance and border layers (mnav_layer_clearance, mnav_layer_border; ClearanceLayer,
// clearance_layer.cpp:67-99 / :122-164, and BorderLayer, border_layer.cpp:66-80 / :104-110, of mesh_layers;
// include/mnav.h).
//
// Clearance: one ray per vertex from p_v along its resident normal, closest hit over the obstacle layer's LBVH
// (mnav_obstacle.h) with the faces that have v as a corner left out; the array is cached on the context and the cost
// pass (computeLethalsAndCosts) runs on every call.  Border: v is a border vertex iff an edge of its CSR row has fewer
// than two incident faces, counted over v's corner table.  Both end in the obstacle layer's diff + compaction scheme,
// extended to compare the cost bits as well as the lethal flag.
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

using mnav_obs::kLeaf;
using mnav_obs::kStack;
using mnav_obs::kCastBlock;
using mnav_obs::kOutBlock;
using mnav_obs::kOutPer;

// counters of one call (device words), in the obstacle layer's layout so that k_obs_scan fills kChanged / kLethal:
// kKept = rays cast, kHits = rays that hit, kOverflow = waves whose traversal stack overflowed
using mnav_obs::kKept;
using mnav_obs::kHits;
using mnav_obs::kOverflow;
using mnav_obs::kChanged;
using mnav_obs::kLethal;
using mnav_obs::kCounters;

// Per-context state: the cached clearance, the border flags and the scratch of the diff; dropped by mnav_upload_mesh.
struct State {
  bool valid = false;            // clr holds the clearance of the resident mesh and normals
  DevBuf<float> clr;             // V
  DevBuf<uint8_t> border;        // V: border flags of the last mnav_layer_border
  DevBuf<uint32_t> ids;          // V: change list
  DevBuf<uint32_t> blk;          // 3 x blocks: changed per block, lethal per block, exclusive offsets
  DevBuf<uint32_t> cnt;          // kCounters words
  uint32_t cast = 0, rays = 0, hits = 0;
  float ms_build = 0.f, ms_cast = 0.f, ms_total = 0.f;
};

struct CastArgs {
  uint32_t V, F, root;
  const float* __restrict__ xyz;
  const float* __restrict__ nrm;
};

// One lane per vertex, in vertex order: the obstacle kernel's closest-hit traversal with the LDS stack, each lane with
// its own RaySetup and slab inverses; faces with v as a corner are skipped at the leaves (Bvh::fvtx).
__global__ __launch_bounds__(kCastBlock) void k_clr_cast(CastArgs A, const float4* __restrict__ nodes, const float4* __restrict__ tris,
                                                         const uint32_t* __restrict__ fvtx, float* __restrict__ clr, uint32_t* __restrict__ cnt)
{
  __shared__ uint32_t stack[kStack * kCastBlock];
  const uint32_t lane = threadIdx.x;
  const uint32_t v = blockIdx.x * kCastBlock + lane;
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
      for (int a = 0; a < 3; ++a) inv[a] = fabsf(n[a]) < 1e-30f ? copysignf(1e30f, n[a]) : 1.0f / n[a];
      uint32_t sp = 0, node = A.root;
      for (;;) {
        if ((node & kLeaf) ? (node & ~kLeaf) >= A.F : node + 1 >= A.F) {
          // not a node of this tree (cannot happen): nothing to test
        } else if (node & kLeaf) {
          const size_t k = node & ~kLeaf;
          const float4 t0 = tris[3 * k], t1 = tris[3 * k + 1], t2 = tris[3 * k + 2];
          const uint32_t f = __float_as_uint(t2.y);
          if (!clr_excluded(v, fvtx[3 * (size_t)f], fvtx[3 * (size_t)f + 1], fvtx[3 * (size_t)f + 2])) {
            const float a[3] = { t0.x, t0.y, t0.z }, b[3] = { t0.w, t1.x, t1.y }, c[3] = { t1.z, t1.w, t2.x };
            float t;
            if (mnav::ray_triangle(rs, o, a, b, c, &t) && (t < best || (t == best && f < best_f))) { best = t; best_f = f; }
          }
        } else {
          const float4 q0 = nodes[4 * (size_t)node], q1 = nodes[4 * (size_t)node + 1], q2 = nodes[4 * (size_t)node + 2], q3 = nodes[4 * (size_t)node + 3];
          const float bl[6] = { q0.x, q0.y, q0.z, q0.w, q1.x, q1.y }, br[6] = { q1.z, q1.w, q2.x, q2.y, q2.z, q2.w };
          float tl, tr;
          const bool hl = mnav_obs::obs_box(bl, o, inv, best, &tl), hr = mnav_obs::obs_box(br, o, inv, best, &tr);
          const uint32_t cl = __float_as_uint(q3.x), cr = __float_as_uint(q3.y);
          if (hl && hr) {
            const uint32_t nearc = tl <= tr ? cl : cr, farc = tl <= tr ? cr : cl;
            if (sp < (uint32_t)kStack) stack[sp++ * kCastBlock + lane] = farc;
            else over = true;
            node = nearc;
            continue;
          }
          if (hl) { node = cl; continue; }
          if (hr) { node = cr; continue; }
        }
        if (sp == 0) break;
        node = stack[--sp * kCastBlock + lane];
      }
      hit = best_f != kNone;
    }
    clr[v] = hit ? best : INFINITY;
  }
  const uint64_t bc = __ballot(cast), bh = __ballot(hit), bo = __ballot(over);
  if (lane == 0) {
    if (bc) atomicAdd(&cnt[kKept], (uint32_t)__popcll(bc));
    if (bh) atomicAdd(&cnt[kHits], (uint32_t)__popcll(bh));
    if (bo) atomicAdd(&cnt[kOverflow], 1u);
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

enum : int { kModeClearance = 0, kModeBorder = 1 };

// where the new cost of a vertex comes from: the cached clearance or the border flags, and the two parameters
struct CostArgs {
  const float* __restrict__ clr;
  const uint8_t* __restrict__ border;
  double p0, p1;                 // robot_height, height_inflation / border_cost, threshold
  uint32_t fresh;                // the slot held no layer: every vertex counts as changed
};

template <int MODE>
__device__ __forceinline__ float clr_new(const CostArgs& A, size_t v, uint8_t* lethal)
{
  if (MODE == kModeClearance) return clr_cost(A.clr[v], A.p0, A.p1, lethal);
  return border_cost_of(A.border[v] != 0, A.p0, A.p1, lethal);
}

// per block of kOutBlock * kOutPer vertices: how many vertices change (lethal flag or cost bits), how many are lethal
template <int MODE>
__global__ __launch_bounds__(kOutBlock) void k_clr_count(uint32_t V, CostArgs A, const float* __restrict__ cost, const uint8_t* __restrict__ lethal,
                                                         uint32_t* __restrict__ blk, uint32_t nblk)
{
  __shared__ uint32_t lds[kOutBlock / 64];
  const size_t v0 = ((size_t)blockIdx.x * kOutBlock + threadIdx.x) * kOutPer;
  uint32_t c = 0, l = 0;
  for (int k = 0; k < kOutPer; ++k)
    if (v0 + k < V) {
      uint8_t f;
      const float x = clr_new<MODE>(A, v0 + k, &f);
      c += A.fresh || f != lethal[v0 + k] || __float_as_uint(x) != __float_as_uint(cost[v0 + k]);
      l += f;
    }
  uint32_t tc, tl;
  (void)mnav_obs::obs_block_scan(c, lds, &tc);
  (void)mnav_obs::obs_block_scan(l, lds, &tl);
  if (threadIdx.x == 0) { blk[blockIdx.x] = tc; blk[nblk + blockIdx.x] = tl; }
}

// the changed ids in ascending order (block offset from k_obs_scan + lane prefix), then the layer's costs and flags
template <int MODE>
__global__ __launch_bounds__(kOutBlock) void k_clr_emit(uint32_t V, CostArgs A, float* __restrict__ cost, uint8_t* __restrict__ lethal,
                                                        const uint32_t* __restrict__ blk, uint32_t nblk, uint32_t* __restrict__ ids)
{
  __shared__ uint32_t lds[kOutBlock / 64];
  const size_t v0 = ((size_t)blockIdx.x * kOutBlock + threadIdx.x) * kOutPer;
  float x[kOutPer];
  uint8_t f[kOutPer], ch[kOutPer];
  uint32_t c = 0;
  for (int k = 0; k < kOutPer; ++k) {
    x[k] = 0.f; f[k] = 0; ch[k] = 0;
    if (v0 + k < V) {
      x[k] = clr_new<MODE>(A, v0 + k, &f[k]);
      ch[k] = A.fresh || f[k] != lethal[v0 + k] || __float_as_uint(x[k]) != __float_as_uint(cost[v0 + k]);
      c += ch[k];
    }
  }
  uint32_t tot;
  uint32_t pos = blk[2 * nblk + blockIdx.x] + mnav_obs::obs_block_scan(c, lds, &tot);
  for (int k = 0; k < kOutPer; ++k) {
    if (v0 + k >= V) break;
    if (ch[k]) ids[pos++] = (uint32_t)(v0 + k);
    lethal[v0 + k] = f[k];
    cost[v0 + k] = x[k];
  }
}

}  // namespace mnav_clr
#endif
