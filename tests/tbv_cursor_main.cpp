// The load cursors of the stream passes of k_tbv_solve (mesh_navigation_amd/csrc/mnav_tbv.h: TBV_LOAD, TBV_SLOAD, TBV_CURSOR_NEXT,
// TBV_CURSORS_INIT, TBV_LOOP), restated in plain C++ and walked on the host: a cursor that leaves the pass's chunks reads foreign
// memory on the device, so the arithmetic is proven here, under the host sanitizers, before a wave runs it.  Built and run alone
// by tests/test_tbv_cursors.py; needs no HIP.
//
// The state is what the assembly keeps in scalar registers:
//   the sequence (s69), the bytes of an order (s75 = chunks per order << 8),
//   the vector cursor {s68 offset, s76 end of its order, s79 entry}: four chunks ahead of the execution, into a ring of four slots,
//   the scalar cursor {s78, s77, s90}: one chunk ahead, into two index sets in turn,
//   the execution: s80 chunks left in the sweep, s84 sweeps done; it has no address of its own -- it consumes ring slot c % 4 and
//   index set c % 2 of the c-th chunk it runs.
// Every load is a real read of a buffer of exactly the pass's size (256 bytes by the vector path, the first 64 of them by the
// scalar path), every chunk carries its own number, and the execution checks that what it consumes is the chunk the sequence
// asks for at that point.  At every sweep boundary -- the sweeps may end at any of them -- what is in flight must be the first
// chunks of the NEXT order of the sequence.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <vector>

#include "../mesh_navigation_amd/csrc/mnav_tbv_seq.h"

namespace {

struct Cursor { uint32_t pos, end, idx; };

struct Pass {
  std::vector<uint32_t> buf;           // the pass's chunks, 64 dwords each: dword 0 (scalar path) and dword 63 (vector path only) = the chunk's number
  uint32_t seq = 0, order_bytes = 0;   // s69, s75
  Cursor v{}, s{};
  uint32_t ring[4][64], iset[2][16];
  unsigned long long fixups = 0;

  void init(uint32_t orders, uint32_t nch, uint32_t sequence)
  {
    buf.assign((size_t)orders * nch * 64u, 0u);
    for (uint32_t c = 0; c < orders * nch; ++c) buf[(size_t)c * 64u] = buf[(size_t)c * 64u + 63u] = c;
    seq = sequence;
    order_bytes = nch << 8;                                            // TBV_CURSORS_INIT
    v.pos = (seq & 3u) * order_bytes; v.end = v.pos + order_bytes; v.idx = 0u;
    s = v;
  }
  void next(Cursor& c)                                                 // TBV_CURSOR_NEXT
  {
    c.idx += 1u;
    c.idx -= c.idx > 15u ? 4u : 0u;
    const uint32_t order = (seq >> (c.idx << 1)) & 3u;
    c.pos = order * order_bytes; c.end = c.pos + order_bytes;
    ++fixups;
  }
  void load(int slot)                                                  // TBV_LOAD
  {
    memcpy(ring[slot], (const char*)buf.data() + v.pos, 256);
    v.pos += 0x100u;
    if (v.pos == v.end) next(v);
  }
  void sload(int set)                                                  // TBV_SLOAD
  {
    memcpy(iset[set], (const char*)buf.data() + s.pos, 64);
    s.pos += 0x100u;
    if (s.pos == s.end) next(s);
  }
};

int fail(const char* what, uint32_t nch, uint32_t seq, unsigned long long sweep, uint32_t chunk)
{
  printf("FAILED: %s (nch %u, sequence 0x%08x, sweep %llu, chunk %u)\n", what, nch, seq, sweep, chunk);
  return 1;
}

// the sweeps: `sweeps` of them (the kernel's cap, or fewer); returns 0 when every consumed and every in-flight chunk is right
int run_sweeps(uint32_t nch, uint32_t seq, uint32_t sweeps, unsigned long long& fixups)
{
  Pass P;
  P.init(4u, nch, seq);
  for (int b = 0; b < 4; ++b) P.load(b);                               // TBV_LOOP
  P.sload(0);
  unsigned long long c = 0;                                            // chunks executed
  for (uint32_t sw = 0; sw < sweeps; ++sw) {
    const uint32_t order = tbv_seq::tbv_seq_at(seq, sw);
    for (uint32_t k = 0; k < nch; ++k, ++c) {                          // TBV_CHUNK
      P.sload((int)((c + 1) & 1));
      const uint32_t want = order * nch + k;
      if (P.ring[c & 3][0] != want || P.ring[c & 3][63] != want) return fail("the ring slot holds another chunk", nch, seq, sw, k);
      if (P.iset[c & 1][0] != want) return fail("the index set holds another chunk", nch, seq, sw, k);
      P.load((int)(c & 3));
    }
    // the sweep boundary: the next four chunks of the sequence are in the ring, the next one's indices in the other set
    for (uint32_t a = 0; a < 4; ++a) {
      const uint32_t sw2 = sw + 1u + a / nch, want = tbv_seq::tbv_seq_at(seq, sw2) * nch + a % nch;
      if (P.ring[(c + a) & 3][0] != want) return fail("in flight at the boundary: not the next order's chunk", nch, seq, sw, a);
    }
    if (P.iset[c & 1][0] != tbv_seq::tbv_seq_at(seq, sw + 1u) * nch) return fail("in flight at the boundary: not the next order's indices", nch, seq, sw, 0);
  }
  fixups += P.fixups;
  return 0;
}

// pre / post: one "order" of the pass's own chunks (the sequence 0), cyclic as before
int run_single(uint32_t nch)
{
  Pass P;
  P.init(1u, nch, 0u);
  for (int b = 0; b < 4; ++b) P.load(b);
  P.sload(0);
  for (uint32_t c = 0; c < nch; ++c) {
    P.sload((int)((c + 1) & 1));
    if (P.ring[c & 3][0] != c || P.iset[c & 1][0] != c) return fail("single pass: another chunk", nch, 0u, 0, c);
    P.load((int)(c & 3));
  }
  return 0;
}

}  // namespace

int main()
{
  // every sequence the builder can produce: it sees the votes only through their order, {0, 1, 2, 3} per entry covers every
  // ranking with and without ties
  std::set<uint32_t> seqs;
  for (uint32_t a = 0; a < 4; ++a) for (uint32_t b = 0; b < 4; ++b) for (uint32_t c = 0; c < 4; ++c) for (uint32_t d = 0; d < 4; ++d)
    seqs.insert(tbv_seq::tbv_seq_build(a, b, c, d));
  for (uint32_t f = 0; f < 4; ++f) seqs.insert(tbv_seq::tbv_seq_rotation(f));
  const uint32_t kCap = 16u * 120u;                                    // the kernel's cap
  const uint32_t nchs[] = { 1u, 2u, 3u, 4u, 5u, 30u, 31u };
  unsigned long long runs = 0, fixups = 0;
  for (uint32_t nch : nchs) {
    if (run_single(nch)) return 1;
    for (uint32_t seq : seqs) {
      if (run_sweeps(nch, seq, kCap, fixups)) return 1;                // (every boundary on the way is checked: any sweep count up to the cap)
      ++runs;
    }
  }
  printf("%zu sequences x %zu chunk counts: %llu runs of %u sweeps, %llu cursor fix-ups, every load inside the pass\n", seqs.size(),
         sizeof(nchs) / sizeof(nchs[0]), runs, kCap, fixups);
  return 0;
}
