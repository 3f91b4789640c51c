// mnav_locate.h -- pose lookup on the device (mnav_locate): MeshMap::getNearestVertexHandle (mesh_map.cpp:1161-1174, a
// nanoflann 1-NN over all vertex positions) and MeshMap::searchContainingFace (:1120-1159) for a batch of positions.
//
// Index: a linear BVH over the vertex POSITIONS (Karras 2012, the hierarchy kernel of mnav_obstacle.h over 64-bit keys).
// The key of a vertex is the 63-bit Morton code of its cell in a grid of 2^21 CUBIC cells per axis over the bounding box
// of the finite vertices (one scale for all axes: a terrain's few decimetres of height must not be cut as finely as its
// hundred metres of ground).  The vertices are sorted by key; a leaf is a run of kRun consecutive ones; every node stores
// the UNPADDED box of its members.  Memory is 24 bytes per vertex whatever the box: an outlier only coarsens the grid (a
// vertex 10^6 m away: 0.5 m cells), equal keys are split by position in the sorted order, and the answers do not depend
// on the tree at all.  Vertices with a non-finite coordinate sort behind all others and are cut off: never candidates.
//
// Search: the answer for a query p is the minimum over all vertices of the packed pair (float bits of d, id),
// d = (dx*dx + dy*dy) + dz*dz in float, dx = p.x - x_v, no contraction; a vertex whose d is +inf or NaN never wins.
// Pruning is exact, not padded: loc_bound evaluates the SAME float expression at the query clamped into the node's box.
// Per axis |p - clamp(p)| <= |p - x_v| for every member v in real numbers, and float subtraction, multiplication and
// addition are monotone under rounding, so bound <= d(v) as floats.  A node is skipped only if bound > best d (strictly:
// an equal bound may hide a lower id) or if the bound is +inf / NaN (then every member's d is, too).
//
// Everything but the kernels compiles for the host as well: tests/test_locate_model.py runs the same descent serially.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "mnav_walk.h"

namespace mnav_loc {

using mnav::kNone;

constexpr uint32_t kLeaf = 0x80000000u;   // child reference: leaf number | kLeaf, else an internal node
constexpr uint32_t kRun = 8;              // vertices per leaf (consecutive in key order)
constexpr int kStack = 32;                // traversal stack per query; a deeper descent falls back to the full scan
constexpr int kLocBlock = 64;             // one wave per workgroup: 16 KiB of LDS stack (node + bound per entry)
constexpr uint64_t kNoKey = ~0ull;        // key of a vertex that is not indexed / packed answer "none"

struct alignas(16) F4 { float x, y, z, w; };

// nodes: (n_leaves - 1) x 4 F4 = left box (lo xyz, hi xyz), right box, left ref, right ref (bits), 2 unused
// pts:   n_leaves * kRun x F4 = position, vertex id (bits), in key order; leaf k = pts[k * kRun .. (k + 1) * kRun); the
//        entries from n_pts on pad the last leaf with NaN positions (their d is NaN: they never win)
struct Index {
  const F4* nodes; const F4* pts;
  uint32_t n_pts, n_leaves, root;
};

MNAV_HD uint32_t loc_root(uint32_t n_leaves) { return n_leaves > 1 ? 0u : (n_leaves == 1 ? kLeaf : kNone); }

MNAV_HD uint64_t loc_expand21(uint64_t v)
{
  v &= 0x1FFFFFull;
  v = (v | v << 32) & 0x001F00000000FFFFull;
  v = (v | v << 16) & 0x001F0000FF0000FFull;
  v = (v | v << 8) & 0x100F00F00F00F00Full;
  v = (v | v << 4) & 0x10C30C30C30C30C3ull;
  v = (v | v << 2) & 0x1249249249249249ull;
  return v;
}
MNAV_HD bool loc_finite(float x, float y, float z)
{
  return (mnav::f2u(x) & 0x7F800000u) != 0x7F800000u && (mnav::f2u(y) & 0x7F800000u) != 0x7F800000u && (mnav::f2u(z) & 0x7F800000u) != 0x7F800000u;
}
// grid cell of coordinate v: lo = the box's lower bound on this axis, scale = the box's largest extent (NaN-free: 0)
MNAV_HD uint32_t loc_cell(float v, float lo, float scale)
{
  const float t = scale > 0.f ? ((v - lo) / scale) * 2097152.f : 0.f;
  return t > 0.f ? (t < 2097151.f ? (uint32_t)t : 2097151u) : 0u;
}
// 63-bit sort key of a position; kNoKey for a position that is not indexed
MNAV_HD uint64_t loc_key(float x, float y, float z, const float lo[3], float scale)
{
  if (!loc_finite(x, y, z)) return kNoKey;
  return loc_expand21(loc_cell(x, lo[0], scale)) << 2 | loc_expand21(loc_cell(y, lo[1], scale)) << 1 | loc_expand21(loc_cell(z, lo[2], scale));
}

// the metric (nanoflann L2_Simple on floats; lvr2 BaseVector::squaredDistanceFrom)
MNAV_HD float loc_d2(const float p[3], float x, float y, float z)
{
  const float dx = p[0] - x, dy = p[1] - y, dz = p[2] - z;
  return (dx * dx + dy * dy) + dz * dz;
}
MNAV_HD float loc_clamp(float p, float lo, float hi) { return p < lo ? lo : (p > hi ? hi : p); }
// lower bound of loc_d2 over every point of the box b = lo xyz, hi xyz (see the header comment)
MNAV_HD float loc_bound(const float p[3], const float b[6])
{
  return loc_d2(p, loc_clamp(p[0], b[0], b[3]), loc_clamp(p[1], b[1], b[4]), loc_clamp(p[2], b[2], b[5]));
}
// may the subtree under a box with this bound hold a better (d, id) than the best d so far?
MNAV_HD bool loc_visit(float bound, float best_d) { return bound <= best_d && bound < INFINITY; }

MNAV_HD uint64_t loc_pack(float d, uint32_t id) { return (uint64_t)mnav::f2u(d) << 32 | id; }

// every vertex of one leaf against the best so far; *cand counts the distances evaluated
MNAV_HD void loc_leaf(const Index& I, uint32_t leaf, const float p[3], uint64_t* best, uint64_t* cand)
{
  const F4* q = I.pts + (size_t)leaf * kRun;
  F4 r[kRun];
  for (uint32_t i = 0; i < kRun; ++i) r[i] = q[i];        // whole leaves: kRun independent loads in flight, no bound to test
  for (uint32_t i = 0; i < kRun; ++i) {
    const float d = loc_d2(p, r[i].x, r[i].y, r[i].z);
    if (d < INFINITY) {                                   // false for NaN as well
      const uint64_t key = loc_pack(d, mnav::f2u(r[i].w));
      if (key < *best) *best = key;
    }
  }
  const uint32_t lo = leaf * kRun;
  *cand += lo + kRun <= I.n_pts ? kRun : I.n_pts - lo;
}

// Exact nearest vertex of p: near child first, the far child is stacked with its bound and tested again when it is
// popped.  `Stack` has bool push(uint32_t node, float bound) (false: full), bool pop(uint32_t*, float*) (false: empty)
// and void clear().  A full stack abandons the descent for a scan of all leaves: the same answer, only slower.
template <class Stack>
MNAV_HD uint64_t loc_nearest(const Index& I, const float p[3], Stack& st, uint64_t* cand)
{
  uint64_t best = kNoKey;
  float best_d = INFINITY;
  uint32_t node = I.root;
  bool over = false;
  st.clear();
  while (node != kNone) {
    if ((node & kLeaf) ? (node & ~kLeaf) >= I.n_leaves : node + 1 >= I.n_leaves) {
      // not a node of this tree (cannot happen): nothing to test
    } else if (node & kLeaf) {
      loc_leaf(I, node & ~kLeaf, p, &best, cand);
      if (best != kNoKey) best_d = mnav::u2f((uint32_t)(best >> 32));
    } else {
      const F4 q0 = I.nodes[4 * (size_t)node], q1 = I.nodes[4 * (size_t)node + 1], q2 = I.nodes[4 * (size_t)node + 2], q3 = I.nodes[4 * (size_t)node + 3];
      const float bl[6] = { q0.x, q0.y, q0.z, q0.w, q1.x, q1.y }, br[6] = { q1.z, q1.w, q2.x, q2.y, q2.z, q2.w };
      const float dl = loc_bound(p, bl), dr = loc_bound(p, br);
      const bool hl = loc_visit(dl, best_d), hr = loc_visit(dr, best_d);
      const uint32_t cl = mnav::f2u(q3.x), cr = mnav::f2u(q3.y);
      if (hl && hr) {
        const bool left_first = dl <= dr;
        if (!st.push(left_first ? cr : cl, left_first ? dr : dl)) { over = true; break; }
        node = left_first ? cl : cr;
        continue;
      }
      if (hl) { node = cl; continue; }
      if (hr) { node = cr; continue; }
    }
    node = kNone;
    uint32_t nn; float nb;
    while (st.pop(&nn, &nb))
      if (loc_visit(nb, best_d)) { node = nn; break; }
  }
  if (over) {
    best = kNoKey;
    for (uint32_t k = 0; k < I.n_leaves; ++k) loc_leaf(I, k, p, &best, cand);
  }
  return best;
}

// MeshMap::searchContainingFace (mesh_map.cpp:1120-1159): the faces of vertex v in getFacesOfVertex row order, the inside
// test of projectedBarycentricCoords (util.cpp:320-347, mnav::walk_bary), the smallest SIGNED distance wins, `<` keeps
// the first face of a tie.  A degenerate face has NaN barycentrics and is never inside.  Nothing found: kNone, zeros.
MNAV_HD uint32_t loc_face(const mnav::WalkMesh& M, uint32_t v, const float p[3], float bary_out[3], float* dist_out)
{
  bary_out[0] = bary_out[1] = bary_out[2] = 0.f; *dist_out = 0.f;
  if (v >= M.V) return kNone;
  float lowest = FLT_MAX;                                               // :1131
  uint32_t best = kNone;
  const mnav::W3 pos = mnav::w3(p[0], p[1], p[2]);
  for (uint32_t i = M.vf_ptr[v]; i < M.vf_ptr[v + 1]; ++i) {            // :1135
    const uint32_t f = M.vf[i];
    if (f >= M.F) continue;
    float bary[3], dist = 0.f;
    if (mnav::walk_bary(M, pos, f, bary, &dist) && dist < lowest) {     // :1140-1142
      lowest = dist; best = f;
      bary_out[0] = bary[0]; bary_out[1] = bary[1]; bary_out[2] = bary[2]; *dist_out = dist;
    }
  }
  return best;
}

#if defined(__HIPCC__)
}  // namespace mnav_loc

#include "mnav_obstacle.h"   // f2ord / ord2f (ordered images of floats for the atomic bounds), k_obs_hierarchy

namespace mnav_loc {
using mnav_obs::f2ord;
using mnav_obs::ord2f;

// Resident index + the buffers of the last call; built by the first mnav_locate after a mesh upload, dropped by the next
// upload and by mnav_destroy.
struct State {
  bool valid = false;
  uint32_t n_pts = 0, n_leaves = 0;
  mnav::DevBuf<F4> nodes, pts;
  mnav::DevBuf<float> q, bary, dist; mnav::DevBuf<uint32_t> vtx, face; size_t cap = 0;   // queries and results of the last call
  mnav::DevBuf<unsigned long long> cnt;                                                  // distances evaluated by the last call
  uint32_t built = 0; float ms_build = 0.f, ms_query = 0.f; uint64_t candidates = 0;
};

// bounds of the finite vertices: bnd[0..2] = ordered min, bnd[3..5] = ordered max (pre-set to 0xFFFFFFFF / 0)
__global__ __launch_bounds__(256) void k_loc_bounds(uint32_t V, const float* __restrict__ xyz, uint32_t* __restrict__ bnd)
{
  float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
  for (uint32_t v = blockIdx.x * 256 + threadIdx.x; v < V; v += gridDim.x * 256) {
    const float p[3] = { xyz[3 * (size_t)v], xyz[3 * (size_t)v + 1], xyz[3 * (size_t)v + 2] };
    if (loc_finite(p[0], p[1], p[2]))
      for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], p[k]); hi[k] = fmaxf(hi[k], p[k]); }
  }
  for (int k = 0; k < 3; ++k)
    for (int off = 32; off > 0; off >>= 1) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], off)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], off)); }
  if ((threadIdx.x & 63) == 0 && lo[0] <= hi[0])
    for (int k = 0; k < 3; ++k) { atomicMin(&bnd[k], f2ord(lo[k])); atomicMax(&bnd[3 + k], f2ord(hi[k])); }
}

// sort keys of all vertices; cnt[0] += vertices with a finite position
__global__ __launch_bounds__(256) void k_loc_keys(uint32_t V, const float* __restrict__ xyz, const uint32_t* __restrict__ bnd,
                                                  uint64_t* __restrict__ keys, uint32_t* __restrict__ ids, uint32_t* __restrict__ cnt)
{
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  bool fin = false;
  if (v < V) {
    const float lo[3] = { ord2f(bnd[0]), ord2f(bnd[1]), ord2f(bnd[2]) };
    const float scale = fmaxf(fmaxf(ord2f(bnd[3]) - lo[0], ord2f(bnd[4]) - lo[1]), ord2f(bnd[5]) - lo[2]);
    const uint64_t k = loc_key(xyz[3 * (size_t)v], xyz[3 * (size_t)v + 1], xyz[3 * (size_t)v + 2], lo, scale);
    keys[v] = k; ids[v] = v;
    fin = k != kNoKey;
  }
  const uint64_t b = __ballot(fin);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(cnt, (uint32_t)__popcll(b));
}

// the indexed vertices in key order (the last leaf padded), and the key of every leaf's first vertex (the hierarchy is
// built over the leaves); one lane per entry of pts
__global__ __launch_bounds__(256) void k_loc_points(uint32_t n_pts, uint32_t n_leaves, const uint32_t* __restrict__ ids, const uint64_t* __restrict__ keys,
                                                    const float* __restrict__ xyz, F4* __restrict__ pts, uint64_t* __restrict__ leaf_keys)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_leaves * kRun) return;
  if (i >= n_pts) { F4 pad; pad.x = pad.y = pad.z = NAN; pad.w = __uint_as_float(kNone); pts[i] = pad; return; }
  const uint32_t v = ids[i];
  F4 q; q.x = xyz[3 * (size_t)v]; q.y = xyz[3 * (size_t)v + 1]; q.z = xyz[3 * (size_t)v + 2]; q.w = __uint_as_float(v);
  pts[i] = q;
  if (i % kRun == 0) leaf_keys[i / kRun] = keys[i];
}

// Leaf k: the box of its vertices, then up the tree as k_obs_leaves does (the second lane to arrive at a node owns its
// union; agent-scope release / acquire around the counter).  No padding: loc_bound needs none.
__global__ __launch_bounds__(256) void k_loc_refit(uint32_t n_pts, uint32_t n_leaves, const F4* __restrict__ pts, F4* nodes,
                                                   const uint32_t* __restrict__ par_int, const uint32_t* __restrict__ par_leaf, uint32_t* arrive)
{
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_leaves || n_leaves < 2) return;
  float box[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
  const uint32_t lo = k * kRun, hi = lo + kRun < n_pts ? lo + kRun : n_pts;
  for (uint32_t i = lo; i < hi; ++i) {
    const F4 q = pts[i];
    box[0] = fminf(box[0], q.x); box[1] = fminf(box[1], q.y); box[2] = fminf(box[2], q.z);
    box[3] = fmaxf(box[3], q.x); box[4] = fmaxf(box[4], q.y); box[5] = fmaxf(box[5], q.z);
  }
  uint32_t child = k | kLeaf;
  uint32_t node = par_leaf[k];
  while (node < n_leaves - 1) {                           // the root's parent is kNone
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

// the traversal stack of one lane: two LDS arrays, entry e of lane l at [e * kLocBlock + l] (conflict-free)
struct LdsStack {
  uint32_t* node; float* bound; uint32_t lane, sp;
  __device__ __forceinline__ void clear() { sp = 0; }
  __device__ __forceinline__ bool push(uint32_t n, float b)
  {
    if (sp >= (uint32_t)kStack) return false;
    node[sp * kLocBlock + lane] = n; bound[sp * kLocBlock + lane] = b; ++sp;
    return true;
  }
  __device__ __forceinline__ bool pop(uint32_t* n, float* b)
  {
    if (sp == 0) return false;
    --sp; *n = node[sp * kLocBlock + lane]; *b = bound[sp * kLocBlock + lane];
    return true;
  }
};

// One lane per query: nearest vertex over the index, then the containing face among that vertex's faces.  Any output
// pointer may be null.
__global__ __launch_bounds__(kLocBlock) void k_loc_query(uint32_t n, const float* __restrict__ q, Index I, mnav::WalkMesh M, uint32_t* __restrict__ vtx_out,
                                                      uint32_t* __restrict__ face_out, float* __restrict__ bary_out, float* __restrict__ dist_out,
                                                      unsigned long long* __restrict__ cnt)
{
  __shared__ uint32_t s_node[kStack * kLocBlock];
  __shared__ float s_bound[kStack * kLocBlock];
  const uint32_t lane = threadIdx.x;
  const uint32_t i = blockIdx.x * kLocBlock + lane;
  uint64_t cand = 0;
  if (i < n) {
    const float p[3] = { q[3 * (size_t)i], q[3 * (size_t)i + 1], q[3 * (size_t)i + 2] };
    LdsStack st{ s_node, s_bound, lane, 0 };
    const uint64_t best = loc_nearest(I, p, st, &cand);
    const uint32_t v = best == kNoKey ? kNone : (uint32_t)best;
    float bary[3], dist;
    const uint32_t f = loc_face(M, v, p, bary, &dist);
    vtx_out[i] = v; face_out[i] = f; dist_out[i] = dist;
    for (int k = 0; k < 3; ++k) bary_out[3 * (size_t)i + k] = bary[k];
  }
  for (int off = 32; off > 0; off >>= 1) cand += __shfl_xor(cand, off);
  if (lane == 0 && cand) atomicAdd(cnt, (unsigned long long)cand);
}

#endif  // __HIPCC__

}  // namespace mnav_loc
