// mnav_obstacle.h -- kernels of the obstacle layer (mnav_layer_obstacle; ObstacleLayer::processPointCloud,
// obstacle_layer.cpp:134-290): a linear BVH over the resident faces (Karras 2012: Morton codes of the face centroids,
// radix sort, hierarchy emission, bottom-up refit with one arrival counter per node), one lane per ray for the
// closest-hit traversal (mnav_ray.h; bvh_closest_hit, which the clearance layer casts with too), then the new lethal set
// is diffed against the layer's old one and compacted into the ascending change list (mnav_changelist.h).  Included by
// mnav.hip after the anonymous namespace of the planner kernels; the C ABI is in mnav_obstacle_capi.h.
#pragma once

#include <rocprim/device/device_radix_sort.hpp>

#include "mnav_changelist.h"
#include "mnav_ray.h"

namespace mnav_obs {

constexpr uint32_t kLeaf = 0x80000000u;   // child reference: leaf (sorted position) | kLeaf, else an internal node
constexpr int kStack = 64;                // traversal stack per lane (LDS): a root-to-leaf path has <= 62 internal nodes
constexpr int kCastBlock = 64;            // one wave per workgroup: 16 KiB of LDS stack

// Resident acceleration structure + per-call scratch of the obstacle layer; built on the first call after a mesh
// upload, dropped by the next upload and by mnav_destroy.
struct Bvh {
  bool valid = false;
  uint32_t F = 0, root = kNone;
  DevBuf<float4> nodes;        // F-1 internal nodes x 4 float4: left box (6 floats), right box (6), left ref, right ref
  DevBuf<float4> tris;         // F leaves in Morton order x 3 float4: a.xyz b.xyz c.xyz, original face id (bits)
  DevBuf<uint32_t> fvtx;       // 3F vertex ids, original face order
  DevBuf<uint8_t> flags;       // V: lethal flags of the current call
  DevBuf<uint8_t> pts; size_t pts_cap = 0;
  float ms_build = 0.f, ms_cast = 0.f, ms_total = 0.f;
  uint32_t kept = 0, hits = 0, lethal_rays = 0;
};

__device__ __forceinline__ uint32_t f2ord(float f)
{
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

// mesh bounds: bnd[0..2] = ordered min, bnd[3..5] = ordered max (pre-set to 0xFFFFFFFF / 0)
__global__ __launch_bounds__(256) void k_obs_bounds(uint32_t V, const float* __restrict__ xyz, uint32_t* __restrict__ bnd)
{
  float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
  for (uint32_t v = blockIdx.x * 256 + threadIdx.x; v < V; v += gridDim.x * 256)
    for (int k = 0; k < 3; ++k) { const float x = xyz[3 * (size_t)v + k]; lo[k] = fminf(lo[k], x); hi[k] = fmaxf(hi[k], x); }
  for (int k = 0; k < 3; ++k)
    for (int off = 32; off > 0; off >>= 1) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], off)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], off)); }
  if ((threadIdx.x & 63) == 0 && lo[0] <= hi[0])
    for (int k = 0; k < 3; ++k) { atomicMin(&bnd[k], f2ord(lo[k])); atomicMax(&bnd[3 + k], f2ord(hi[k])); }
}

__device__ __forceinline__ uint32_t expand10(uint32_t v)
{
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}

// 30-bit Morton code of every face centroid; ids = 0..F-1
__global__ __launch_bounds__(256) void k_obs_morton(uint32_t F, const uint32_t* __restrict__ fv, const float* __restrict__ xyz,
                                                     const uint32_t* __restrict__ bnd, uint32_t* __restrict__ keys, uint32_t* __restrict__ ids)
{
  const uint32_t f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  uint32_t code = 0;
  for (int k = 0; k < 3; ++k) {
    const float c = (xyz[3 * (size_t)fv[3 * (size_t)f] + k] + xyz[3 * (size_t)fv[3 * (size_t)f + 1] + k] + xyz[3 * (size_t)fv[3 * (size_t)f + 2] + k]) * (1.0f / 3.0f);
    const float lo = ord2f(bnd[k]), ext = ord2f(bnd[3 + k]) - lo;
    float u = ext > 0.f ? (c - lo) / ext : 0.f;
    u = fminf(fmaxf(u * 1024.f, 0.f), 1023.f);          // NaN-free: fmaxf(NaN, 0) = 0
    code |= expand10((uint32_t)u) << (2 - k);
  }
  keys[f] = code;
  ids[f] = f;
}

// Karras 2012 common-prefix length of sorted keys i and j (index as tie-break), -1 outside [0, F).  Key = uint32_t (the
// faces here) or uint64_t (the vertex index of mnav_locate.h).
template <class Key>
__device__ __forceinline__ int obs_delta(const Key* __restrict__ keys, int64_t F, int64_t i, int64_t j)
{
  if (j < 0 || j >= F) return -1;
  const Key a = keys[i], b = keys[j];
  if (a == b) return 8 * (int)sizeof(Key) + __clz((uint32_t)i ^ (uint32_t)j);
  if constexpr (sizeof(Key) == 8) return __clzll((long long)(a ^ b));
  else return __clz((uint32_t)(a ^ b));
}

// internal node i covers a key range; its split is where the common prefix grows (Karras 2012, Fig. 4)
template <class Key>
__global__ __launch_bounds__(256) void k_obs_hierarchy(uint32_t F, const Key* __restrict__ keys, float4* __restrict__ nodes,
                                                       uint32_t* __restrict__ par_int, uint32_t* __restrict__ par_leaf)
{
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n = F;
  if (i >= n - 1) return;
  const int d = obs_delta(keys, n, i, i + 1) - obs_delta(keys, n, i, i - 1) >= 0 ? 1 : -1;
  const int dmin = obs_delta(keys, n, i, i - d);
  int64_t lmax = 2;
  while (obs_delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
  int64_t l = 0;
  for (int64_t t = lmax / 2; t >= 1; t /= 2)
    if (obs_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
  const int64_t j = i + l * d;
  const int dnode = obs_delta(keys, n, i, j);
  int64_t s = 0, t = l;
  do {
    t = (t + 1) >> 1;
    if (obs_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
  } while (t > 1);
  const int64_t gamma = i + s * d + (d < 0 ? -1 : 0);
  if (gamma < 0 || gamma > n - 2) return;                // cannot happen for sorted keys; keeps every write in bounds
  const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
  const uint32_t left = lo == gamma ? ((uint32_t)gamma | kLeaf) : (uint32_t)gamma;
  const uint32_t right = hi == gamma + 1 ? ((uint32_t)(gamma + 1) | kLeaf) : (uint32_t)(gamma + 1);
  uint32_t* w = (uint32_t*)(nodes + 4 * i);
  w[12] = left; w[13] = right; w[14] = 0; w[15] = 0;
  if (left & kLeaf) par_leaf[left & ~kLeaf] = (uint32_t)i; else par_int[left] = (uint32_t)i;
  if (right & kLeaf) par_leaf[right & ~kLeaf] = (uint32_t)i; else par_int[right] = (uint32_t)i;
  if (i == 0) par_int[0] = kNone;
}

// Leaf k: the triangle in Morton order, its box padded by 1e-4 (1 + max |coordinate|) on every side, so that no
// rounding of the slab test or of the watertight test can cull a face the test hits (brute force == BVH, bit for bit);
// then up the tree: the second lane to arrive at a node owns its union (agent-scope release / acquire around the counter).
__global__ __launch_bounds__(256) void k_obs_leaves(uint32_t F, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ fv,
                                                    const float* __restrict__ xyz, float4* __restrict__ tris, float4* nodes,
                                                    const uint32_t* __restrict__ par_int, const uint32_t* __restrict__ par_leaf,
                                                    uint32_t* arrive)
{
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= F) return;
  const uint32_t f = ids[k];
  float p[9];
  for (int c = 0; c < 3; ++c)
    for (int a = 0; a < 3; ++a) p[3 * c + a] = xyz[3 * (size_t)fv[3 * (size_t)f + c] + a];
  tris[3 * (size_t)k + 0] = make_float4(p[0], p[1], p[2], p[3]);
  tris[3 * (size_t)k + 1] = make_float4(p[4], p[5], p[6], p[7]);
  tris[3 * (size_t)k + 2] = make_float4(p[8], __uint_as_float(f), 0.f, 0.f);
  if (F == 1) return;
  float box[6];
  float m = 0.f;
  for (int a = 0; a < 3; ++a) {
    box[a] = fminf(fminf(p[a], p[3 + a]), p[6 + a]);
    box[3 + a] = fmaxf(fmaxf(p[a], p[3 + a]), p[6 + a]);
    m = fmaxf(m, fmaxf(fabsf(box[a]), fabsf(box[3 + a])));
  }
  const float pad = 1e-4f * (1.f + m);
  for (int a = 0; a < 3; ++a) { box[a] -= pad; box[3 + a] += pad; }
  uint32_t child = k | kLeaf;
  uint32_t node = par_leaf[k];
  while (node < F - 1) {                                // the root's parent is kNone
    float* w = (float*)(nodes + 4 * (size_t)node);
    const uint32_t side = __float_as_uint(w[12]) == child ? 0 : 6;
    for (int a = 0; a < 6; ++a) w[side + a] = box[a];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t old = __hip_atomic_fetch_add(&arrive[node], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == 0) return;                                 // the sibling's lane finishes this node
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const volatile float* r = w;
    for (int a = 0; a < 3; ++a) {
      box[a] = fminf(r[a], r[6 + a]);
      box[3 + a] = fmaxf(r[3 + a], r[9 + a]);
    }
    child = node;
    node = par_int[node];
  }
}

// slab test of a padded box; the far bound is widened by 1 + 2 gamma_3 (Ize 2013) against the test's own rounding
__device__ __forceinline__ bool obs_box(const float* b, const float o[3], const float inv[3], float best, float* tnear)
{
  float tn = 0.f, tf = INFINITY;
  for (int a = 0; a < 3; ++a) {
    const float t0 = (b[a] - o[a]) * inv[a], t1 = (b[3 + a] - o[a]) * inv[a];
    tn = fmaxf(tn, fminf(t0, t1));
    tf = fminf(tf, fmaxf(t0, t1));
  }
  *tnear = tn;
  return tn <= tf * 1.000001f && tn <= best;
}

// closest hit of one ray over the BVH (ties: smallest face id); `skip(f)` leaves face f out.  Returns true on a stack overflow.
template <class Skip>
__device__ __forceinline__ bool bvh_closest_hit(uint32_t F, uint32_t root, const float4* __restrict__ nodes, const float4* __restrict__ tris,
                                                const RaySetup& rs, const float* o, const float* inv, uint32_t* stack, uint32_t lane, Skip skip,
                                                float* best_out, uint32_t* best_f_out)
{
  bool over = false;
  float best = INFINITY;
  uint32_t best_f = kNone, sp = 0, node = root;
  for (;;) {
    if ((node & kLeaf) ? (node & ~kLeaf) >= F : node + 1 >= F) {
      // not a node of this tree (cannot happen): nothing to test
    } else if (node & kLeaf) {
      const size_t k = node & ~kLeaf;
      const float4 t0 = tris[3 * k], t1 = tris[3 * k + 1], t2 = tris[3 * k + 2];
      const uint32_t f = __float_as_uint(t2.y);
      if (!skip(f)) {
        const float a[3] = { t0.x, t0.y, t0.z }, b[3] = { t0.w, t1.x, t1.y }, c[3] = { t1.z, t1.w, t2.x };
        float t;
        if (ray_triangle(rs, o, a, b, c, &t) && (t < best || (t == best && f < best_f))) { best = t; best_f = f; }
      }
    } else {
      const float4 q0 = nodes[4 * (size_t)node], q1 = nodes[4 * (size_t)node + 1], q2 = nodes[4 * (size_t)node + 2], q3 = nodes[4 * (size_t)node + 3];
      const float bl[6] = { q0.x, q0.y, q0.z, q0.w, q1.x, q1.y }, br[6] = { q1.z, q1.w, q2.x, q2.y, q2.z, q2.w };
      float tl, tr;
      const bool hl = obs_box(bl, o, inv, best, &tl), hr = obs_box(br, o, inv, best, &tr);
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
  *best_out = best; *best_f_out = best_f;
  return over;
}

struct CastArgs {
  uint32_t n, step, F, root;
  float m[12];
  float inv[3];
  RaySetup rs;
  double max_dist, robot_height;
};

// One lane per ray: gather the point (byte stride), filter, transform, closest hit over the BVH (ties: smallest face id),
// lethal -> the face's three vertices are flagged (plain byte stores of 1: no race that matters).
__global__ __launch_bounds__(kCastBlock) void k_obs_cast(CastArgs A, const uint8_t* __restrict__ pts, const float4* __restrict__ nodes,
                                                         const float4* __restrict__ tris, const uint32_t* __restrict__ fvtx,
                                                         uint8_t* __restrict__ flags, uint32_t* __restrict__ cnt)
{
  __shared__ uint32_t stack[kStack * kCastBlock];
  const uint32_t lane = threadIdx.x;
  const uint32_t i = blockIdx.x * kCastBlock + lane;
  bool kept = false, hit = false, leth = false, over = false;
  if (i < A.n) {
    const uint8_t* p = pts + (size_t)i * A.step;
    float x, y, z;
    if ((A.step & 3u) == 0) { const float* q = (const float*)p; x = q[0]; y = q[1]; z = q[2]; }
    else { __builtin_memcpy(&x, p, 4); __builtin_memcpy(&y, p + 4, 4); __builtin_memcpy(&z, p + 8, 4); }
    kept = ray_point_kept(x, y, z, A.max_dist);
    float o[3];
    ray_transform(A.m, x, y, z, o);
    if (kept && A.F && ray_origin_finite(o)) {
      float best; uint32_t best_f;
      over = bvh_closest_hit(A.F, A.root, nodes, tris, A.rs, o, A.inv, stack, lane, [](uint32_t) { return false; }, &best, &best_f);
      if (best_f != kNone) {
        hit = true;
        if ((double)best <= A.robot_height) {
          leth = true;
          for (int c = 0; c < 3; ++c) flags[fvtx[3 * (size_t)best_f + c]] = 1;
        }
      }
    }
  }
  const uint64_t bk = __ballot(kept), bh = __ballot(hit), bl = __ballot(leth), bo = __ballot(over);
  if (lane == 0) {
    if (bk) atomicAdd(&cnt[mnav_chg::kKept], (uint32_t)__popcll(bk));
    if (bh) atomicAdd(&cnt[mnav_chg::kHits], (uint32_t)__popcll(bh));
    if (bl) atomicAdd(&cnt[mnav_chg::kLethalRays], (uint32_t)__popcll(bl));
    if (bo) atomicAdd(&cnt[mnav_chg::kOverflow], 1u);
  }
}

// change-list rule: the flags of this call are the slot's new lethal set, cost +inf / 0; a vertex changed iff its flag did
struct FlagRule {
  static constexpr bool kCostBits = false;
  const uint8_t* __restrict__ flags;
  __device__ __forceinline__ float operator()(size_t v, uint8_t* lethal) const
  {
    *lethal = flags[v];
    return *lethal ? INFINITY : 0.f;
  }
};

}  // namespace mnav_obs
