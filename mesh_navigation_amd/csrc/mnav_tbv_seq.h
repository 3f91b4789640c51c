// mnav_tbv_seq.h -- the sequence of sweep orders of one activation of k_tbv_solve (mnav_tbv.h), for the host and the device.
// Stands alone: a host compiler takes it without HIP (tests/tbv_seq_shim.cpp, tests/tbv_cursor_main.cpp).
//
// A tile's sweep stream holds the same edges in four orders.  After the ghosts -> owned pass every lane in which a ghost lowered a
// row names the order that runs with a wave entering at that row; the kernel counts the votes per order by ballot.  The sequence:
//   * first the orders with at least one vote, by votes descending, ties to the lower order;
//   * from there the rotation: last voted order + 1, + 2, ... mod 4, for as long as sweeps are needed;
//   * no vote at all (the wave source's tile): the rotation from order 0.
// Which orders run, and how often, changes no bit of the result: the sweeps end on the first sweep that changes nothing in any
// lane, and such a sweep of ANY order proves the tile-local fixed point.
//
// Packing: sixteen 2-bit entries in one word, entry k in bits 2 k + 1 : 2 k.  At most four orders are voted for, so entries 4 .. 15
// are rotation: entry k equals entry k - 4 from k = 8 on, and an index past 15 steps back by 4 (tbv_seq_index).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MNAV_SEQ_HD __host__ __device__ inline
#else
#define MNAV_SEQ_HD inline
#endif

namespace tbv_seq {

constexpr uint32_t kEntries = 16;

// the index of the entry after entry `k` (k <= 15): the kernel's cursors step exactly like this
MNAV_SEQ_HD uint32_t tbv_seq_next_index(uint32_t k) { return k + 1u > 15u ? k + 1u - 4u : k + 1u; }
// the stored entry that sweep number `k` (any k) runs
MNAV_SEQ_HD uint32_t tbv_seq_index(uint32_t k) { return k < kEntries ? k : 12u + (k & 3u); }
MNAV_SEQ_HD uint32_t tbv_seq_at(uint32_t seq, uint32_t k) { return (seq >> (2u * tbv_seq_index(k))) & 3u; }

// order `first`, then the rotation: what the kernel ran before the sequence existed (option tb_sweep_seq = 0, mnav_debug_tbv_sweeps).
// The rotation from 0 is 0, 1, 2, 3 = 0xE4 in every byte; from `first` it is that pattern moved down by `first` entries.
MNAV_SEQ_HD uint32_t tbv_seq_rotation(uint32_t first) { return (uint32_t)(0xE4E4E4E4E4E4E4E4ull >> (2u * (first & 3u))); }

// the sequence from the votes per order: straight-line scalar code on the device (a few dozen instructions per work item)
MNAV_SEQ_HD uint32_t tbv_seq_build(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3)
{
  // key = votes << 2 | 3 - order: a larger key is an order with more votes, the lower order on a tie.  The keys are distinct, and
  // those of the n voted orders (>= 4) lie above the others (<= 3).
  uint32_t k0 = (c0 << 2) | 3u, k1 = (c1 << 2) | 2u, k2 = (c2 << 2) | 1u, k3 = c3 << 2;
  const uint32_t n = (c0 != 0u) + (c1 != 0u) + (c2 != 0u) + (c3 != 0u);
  // descending, by the sorting network (0,1) (2,3) (0,2) (1,3) (1,2): the n voted orders come first
#define MNAV_SEQ_CX(a, b) { const uint32_t hi = a > b ? a : b, lo = a > b ? b : a; a = hi; b = lo; }
  MNAV_SEQ_CX(k0, k1) MNAV_SEQ_CX(k2, k3) MNAV_SEQ_CX(k0, k2) MNAV_SEQ_CX(k1, k3) MNAV_SEQ_CX(k1, k2)
#undef MNAV_SEQ_CX
  const uint32_t all = (~k0 & 3u) | (~k1 & 3u) << 2 | (~k2 & 3u) << 4 | (~k3 & 3u) << 6;     // (order = 3 - key bits 1:0)
  const uint32_t prefix = all & ((1u << (2u * n)) - 1u);
  const uint32_t next = n ? ((all >> (2u * n - 2u)) + 1u) & 3u : 0u;   // the rotation goes on behind the last voted order; no vote: from order 0
  return prefix | tbv_seq_rotation(next) << (2u * n);
}

}  // namespace tbv_seq
