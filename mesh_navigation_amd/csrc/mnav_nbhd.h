// mnav_nbhd.h -- the local-neighbourhood layers (mnav_layer_height_diff / _roughness / _ridge; HeightDiffLayer,
// RoughnessLayer, RidgeLayer of mesh_layers): per vertex v a visit of N(v), the connected component of v in the subgraph
// of the mesh edges induced by the open ball of `radius` around v, and one reduction over it (include/mnav.h, DESIGN.md
// §3.5).
//
// The per-pair rules (ball test, the two terms, the fixed-point conversion of a term) are MNAV_HD functions written out
// operation by operation: the library and the CPU test shim are built with -ffp-contract=off, and tests/nbhd_model.py
// restates the same sequence in numpy float32.  nb_centre_host is the same visit for one centre, single-threaded, on the
// host (tests, tools/gpu_nbhd_perf.py).  The kernels below it are device only.
//
// Kernels: a group of kGroup lanes owns one centre; the group's LDS holds an open-addressing hash set of vertex ids and
// the member list, which is also the visit queue: a vertex is appended exactly once, by the lane whose hash insert
// succeeded, and that lane adds its term.  A centre whose neighbourhood outgrows the LDS cap goes to a spill list; a
// second k_nbhd pass with a 4x larger cap takes that list, and k_nbhd_spill finishes what outgrows it too with one wave
// per centre and the same state in global scratch; the host grows the scratch for the few that outgrow that (a capacity
// of V cannot overflow).
#pragma once

#include <math.h>
#include <stdint.h>

#include "mnav_eval.h"   // MNAV_HD, acosf_ref

namespace mnav_nb {

enum : int { kHeight = 0, kRough = 1, kRidge = 2 };

constexpr double kFix = 4294967296.0;          // 2^32: terms are summed as int64 multiples of 2^-32
constexpr double kUnfix = 1.0 / 4294967296.0;

// squared distance of u from v, lvr2 BaseVector::squaredDistanceFrom order: (dx*dx + dy*dy) + dz*dz, d = u - v
MNAV_HD float nb_d2(float vx, float vy, float vz, float ux, float uy, float uz)
{
  const float dx = ux - vx, dy = uy - vy, dz = uz - vz;
  const float xy = dx * dx + dy * dy;
  return xy + dz * dz;
}
// the open ball: strict, compared in double against radius * radius in double
MNAV_HD bool nb_in_ball(float vx, float vy, float vz, float ux, float uy, float uz, double r2)
{
  return (double)nb_d2(vx, vy, vz, ux, uy, uz) < r2;
}
// roughness term: acos of the normals' dot product (ax*bx + ay*by) + az*bz, clamped to [-1, 1] (the clamp is the
// library's choice: lvr2's handling of |dot| > 1 is not known)
MNAV_HD float nb_rough_term(float ax, float ay, float az, float bx, float by, float bz)
{
  const float xy = ax * bx + ay * by;
  float d = xy + az * bz;
  d = d > 1.0f ? 1.0f : (d < -1.0f ? -1.0f : d);
  return mnav::acosf_ref(d);
}
// ridge term (ridge_layer.cpp:170-172): |(p_u + n_u) - (p_v + n_v)| with the squared length in the order of nb_d2
MNAV_HD float nb_ridge_term(float pvx, float pvy, float pvz, float nvx, float nvy, float nvz,
                            float pux, float puy, float puz, float nux, float nuy, float nuz)
{
  const float rx = pvx + nvx, ry = pvy + nvy, rz = pvz + nvz;
  const float cx = pux + nux, cy = puy + nuy, cz = puz + nuz;
  return sqrtf(nb_d2(rx, ry, rz, cx, cy, cz));
}
// a term as a fixed-point integer: llrint((double)t * 2^32), rounded half to even
MNAV_HD long long nb_fixed(float t) { return (long long)rint((double)t * kFix); }
// mean of n terms whose fixed-point sum is s
MNAV_HD float nb_mean(long long s, uint32_t n) { return (float)(((double)s * kUnfix) / (double)n); }

#if !defined(__HIP_DEVICE_COMPILE__)
// One centre on the host, single-threaded: the same set N(v) and the same reduction as the kernels.  `stamp` is a V-sized
// scratch array, `queue` a scratch list; stamp[u] == tag marks a member (tags must differ between calls).
inline float nb_centre_host(int op, uint32_t v, const uint32_t* row_ptr, const uint32_t* nbr, const float* xyz, const float* nrm,
                            double r2, uint32_t* stamp, uint32_t tag, uint32_t* queue, uint32_t* size_out)
{
  const float* pv = xyz + 3 * (size_t)v;
  const float* nv = nrm ? nrm + 3 * (size_t)v : nullptr;
  uint32_t tail = 0;
  float lo = pv[2], hi = pv[2];
  long long s = 0;
  auto add = [&](uint32_t u) {
    stamp[u] = tag;
    queue[tail++] = u;
    const float* pu = xyz + 3 * (size_t)u;
    if (op == kHeight) { lo = pu[2] < lo ? pu[2] : lo; hi = pu[2] > hi ? pu[2] : hi; }
    else if (op == kRough) { const float* nu = nrm + 3 * (size_t)u; s += nb_fixed(nb_rough_term(nv[0], nv[1], nv[2], nu[0], nu[1], nu[2])); }
    else {
      const float* nu = nrm + 3 * (size_t)u;
      s += nb_fixed(nb_ridge_term(pv[0], pv[1], pv[2], nv[0], nv[1], nv[2], pu[0], pu[1], pu[2], nu[0], nu[1], nu[2]));
    }
  };
  add(v);
  for (uint32_t head = 0; head < tail; ++head) {
    const uint32_t m = queue[head];
    for (uint32_t k = row_ptr[m]; k < row_ptr[m + 1]; ++k) {
      const uint32_t u = nbr[k];
      if (stamp[u] == tag) continue;
      const float* pu = xyz + 3 * (size_t)u;
      if (nb_in_ball(pv[0], pv[1], pv[2], pu[0], pu[1], pu[2], r2)) add(u);
    }
  }
  if (size_out) *size_out = tail;
  return op == kHeight ? hi - lo : nb_mean(s, tail);
}
#endif

}  // namespace mnav_nb

#if defined(__HIPCC__)
namespace mnav_nb {

constexpr int kGroup = 16;                    // lanes per centre on the LDS path: 4 centres per wave
constexpr int kNbBlock = 256;                 // 16 centres per workgroup
constexpr int kCentresPerBlock = kNbBlock / kGroup;
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr uint32_t kDefaultLdsCap = 128;      // members per centre in LDS, first pass (24 KiB per workgroup)
constexpr uint32_t kWideLdsCap = 512;         // second LDS pass over the first one's spill list (96 KiB per workgroup)
// counters of one call (device words): spilled centres, centres that overflowed the spill scratch, sum of |N(v)|, max |N(v)|
enum { kSpilled = 0, kOverflow = 1, kMaxSize = 2, kCounters32 = 4 };

// Per-context state: the device counters, spill lists and scratch; dropped by mnav_upload_mesh and mnav_destroy.
struct State {
  DevBuf<uint32_t> cnt;                       // kCounters32 words + one 64-bit visit sum
  DevBuf<uint32_t> list[2];                   // spill list / overflow list (V entries each)
  DevBuf<uint32_t> scratch; size_t scratch_words = 0;
  uint32_t centres = 0, max_size = 0, spilled = 0; uint64_t visits = 0; float ms = 0.f;
};

struct Mesh {
  const uint32_t* __restrict__ row_ptr; const uint32_t* __restrict__ nbr; const float* __restrict__ xyz; const float* __restrict__ nrm;
  uint32_t V; double r2; double threshold;
};

// what a lane accumulates over the members it inserted
struct Acc { float lo, hi; long long s; };

template <int OP>
__device__ __forceinline__ void nb_add(Acc& a, const Mesh& M, const float* pv, const float* nv, uint32_t u, float ux, float uy, float uz)
{
  if (OP == kHeight) { a.lo = fminf(a.lo, uz); a.hi = fmaxf(a.hi, uz); return; }
  const float nux = M.nrm[3 * (size_t)u], nuy = M.nrm[3 * (size_t)u + 1], nuz = M.nrm[3 * (size_t)u + 2];
  if (OP == kRough) a.s += nb_fixed(nb_rough_term(nv[0], nv[1], nv[2], nux, nuy, nuz));
  else a.s += nb_fixed(nb_ridge_term(pv[0], pv[1], pv[2], nv[0], nv[1], nv[2], ux, uy, uz, nux, nuy, nuz));
}

// Insert u into the hash set (linear probing, hmask + 1 slots).  1 = inserted, 0 = already there, -1 = no free slot met
// within the probe bound (cannot happen while the set is at most half full; the caller treats it as an overflow).
template <class P>
__device__ __forceinline__ int nb_insert(P hash, uint32_t hmask, uint32_t u)
{
  uint32_t h = (u * 0x9E3779B1u) & hmask;
  for (uint32_t probe = 0; probe <= hmask; ++probe) {
    const uint32_t old = atomicCAS(&hash[h], kEmpty, u);
    if (old == kEmpty) return 1;
    if (old == u) return 0;
    h = (h + 1) & hmask;
  }
  return -1;
}

// The lanes of one group hand each other what they wrote (members, hash entries) between rounds.  LDS (G < 64) is
// ordered at wavefront scope; the spill path's global scratch (G == 64) needs agent scope, so that no lane reads a stale
// L1 line of a member another lane stored.
template <int G>
__device__ __forceinline__ void nb_sync()
{
  if (G == 64) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (G == 64) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); else __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The visit of one centre by a group of G lanes (lane = 0..G-1; gbase = the group's first lane in the wave).  The hash set
// must be empty.  Returns |N(v)| and leaves the group's reduced value in `value`, or returns 0 on overflow (more than cap
// members).
template <int OP, int G, class P>
__device__ __forceinline__ uint32_t nb_visit(const Mesh& M, uint32_t v, uint32_t lane, uint32_t gbase, P hash, uint32_t hmask, P mem,
                                             uint32_t cap, float& value)
{
  const float pv[3] = { M.xyz[3 * (size_t)v], M.xyz[3 * (size_t)v + 1], M.xyz[3 * (size_t)v + 2] };
  float nv[3] = { 0.f, 0.f, 0.f };
  if (OP != kHeight) { nv[0] = M.nrm[3 * (size_t)v]; nv[1] = M.nrm[3 * (size_t)v + 1]; nv[2] = M.nrm[3 * (size_t)v + 2]; }
  Acc a{ INFINITY, -INFINITY, 0 };
  if (lane == 0) {
    __hip_atomic_store(&hash[(v * 0x9E3779B1u) & hmask], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&mem[0], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    nb_add<OP>(a, M, pv, nv, v, pv[0], pv[1], pv[2]);
  }
  nb_sync<G>();
  const unsigned long long gmask = (G == 64) ? ~0ull : (((1ull << G) - 1ull) << gbase);
  const unsigned long long below = (1ull << (gbase + lane)) - 1ull;
  uint32_t head = 0, tail = 1;
  bool over = false;
  while (head < tail && !over) {
    const uint32_t end = head + G < tail ? head + G : tail;        // this round: members head .. end-1, one per lane
    const uint32_t idx = head + lane;
    uint32_t b = 0, e = 0;
    if (idx < end) {
      const uint32_t m = __hip_atomic_load(&mem[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      b = M.row_ptr[m]; e = M.row_ptr[m + 1];
    }
    uint32_t deg = e - b;
    for (int off = G / 2; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(deg, off, G); deg = o > deg ? o : deg; }
    for (uint32_t j = 0; j < deg; ++j) {
      bool ins = false;
      float ux = 0.f, uy = 0.f, uz = 0.f;
      uint32_t u = 0;
      if (b + j < e) {
        u = M.nbr[b + j];
        ux = M.xyz[3 * (size_t)u]; uy = M.xyz[3 * (size_t)u + 1]; uz = M.xyz[3 * (size_t)u + 2];
        if (nb_in_ball(pv[0], pv[1], pv[2], ux, uy, uz, M.r2)) {
          const int r = nb_insert(hash, hmask, u);
          ins = r == 1;
          over = r < 0;
        }
      }
      const unsigned long long bal = __ballot(ins) & gmask;
      const uint32_t n = (uint32_t)__popcll(bal);
      over = (__ballot(over) & gmask) != 0ull || tail + n > cap;
      if (over) break;
      if (ins) {
        __hip_atomic_store(&mem[tail + (uint32_t)__popcll(bal & below)], u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        nb_add<OP>(a, M, pv, nv, u, ux, uy, uz);
      }
      tail += n;
    }
    nb_sync<G>();
    head = end;
  }
  if (over) return 0;
  for (int off = G / 2; off > 0; off >>= 1) {
    if (OP == kHeight) { a.lo = fminf(a.lo, __shfl_xor(a.lo, off, G)); a.hi = fmaxf(a.hi, __shfl_xor(a.hi, off, G)); }
    else a.s += __shfl_xor(a.s, off, G);
  }
  value = OP == kHeight ? a.hi - a.lo : nb_mean(a.s, tail);
  return tail;
}

__device__ __forceinline__ void nb_store(const Mesh& M, uint32_t v, float value, float* __restrict__ cost, uint8_t* __restrict__ lethal)
{
  cost[v] = value;
  lethal[v] = ((double)value > M.threshold) ? 1 : 0;
}

// LDS path: kCentresPerBlock consecutive centres per workgroup (centre i = list[i], or i without a list; n centres), one
// group of kGroup lanes each.  Dynamic LDS: per group hmask + 1 hash words, then cap member words.  A centre with more than
// cap members is appended to `spill` (count in cnt[ctr]).
template <int OP>
__global__ __launch_bounds__(kNbBlock) void k_nbhd(Mesh M, const uint32_t* __restrict__ list, uint32_t n_centres, uint32_t hmask, uint32_t cap,
                                                  float* __restrict__ cost, uint8_t* __restrict__ lethal, uint32_t* __restrict__ spill,
                                                  uint32_t* __restrict__ cnt, uint32_t ctr)
{
  extern __shared__ uint32_t nb_lds[];
  __shared__ uint32_t blk_max;
  __shared__ unsigned long long blk_sum;
  const uint32_t g = threadIdx.x / kGroup, lane = threadIdx.x % kGroup, gbase = (threadIdx.x & 63u) & ~(uint32_t)(kGroup - 1);
  const uint32_t words = hmask + 1 + cap;
  uint32_t* hash = nb_lds + (size_t)g * words;
  uint32_t* mem = hash + hmask + 1;
  if (threadIdx.x == 0) { blk_max = 0; blk_sum = 0; }
  for (uint32_t i = lane; i <= hmask; i += kGroup) hash[i] = kEmpty;
  __syncthreads();
  const uint32_t i = blockIdx.x * kCentresPerBlock + g;
  if (i < n_centres) {
    const uint32_t v = list ? list[i] : i;
    float value = 0.f;
    const uint32_t n = nb_visit<OP, kGroup>(M, v, lane, gbase, hash, hmask, mem, cap, value);
    if (lane == 0) {
      if (n) {
        nb_store(M, v, value, cost, lethal);
        atomicAdd(&blk_sum, (unsigned long long)n);
        atomicMax(&blk_max, n);
      } else {
        spill[atomicAdd(&cnt[ctr], 1u)] = v;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && blk_sum) {
    atomicAdd((unsigned long long*)(cnt + kCounters32), blk_sum);
    atomicMax(&cnt[kMaxSize], blk_max);
  }
}

// Spill path: one wave per centre of `list` (n entries), its hash set (hmask + 1 words) and member list (cap words) in
// the wave's slice of `scratch`; the grid's waves take the centres in turn.  A centre that outgrows `cap` here too is
// appended to `over` for a pass with a larger capacity.
template <int OP>
__global__ __launch_bounds__(64) void k_nbhd_spill(Mesh M, const uint32_t* __restrict__ list, uint32_t n, uint32_t hmask, uint32_t cap,
                                                   uint32_t* __restrict__ scratch, float* __restrict__ cost, uint8_t* __restrict__ lethal,
                                                   uint32_t* __restrict__ over, uint32_t* __restrict__ cnt)
{
  const uint32_t lane = threadIdx.x;
  uint32_t* hash = scratch + (size_t)blockIdx.x * (hmask + 1 + (size_t)cap);
  uint32_t* mem = hash + hmask + 1;
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t v = list[i];
    for (uint32_t k = lane; k <= hmask; k += 64) __hip_atomic_store(&hash[k], kEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    nb_sync<64>();
    float value = 0.f;
    const uint32_t s = nb_visit<OP, 64>(M, v, lane, 0, hash, hmask, mem, cap, value);
    if (lane == 0) {
      if (s) {
        nb_store(M, v, value, cost, lethal);
        atomicAdd((unsigned long long*)(cnt + kCounters32), (unsigned long long)s);
        atomicMax(&cnt[kMaxSize], s);
      } else {
        over[atomicAdd(&cnt[kOverflow], 1u)] = v;
      }
    }
  }
}

}  // namespace mnav_nb
#endif
