// Walks the record of the resident outputs (csrc/mnav_resident.h) through every transition and prints after each step whether
// the claim "the slots hold what the tile-batch engine's last finalize pass wrote" stands, for how many slots and with vector
// maps or not.  tests/test_finalize_claim.py builds this file alone, with the host sanitizers, runs it and compares the lines
// with its table.
//
//   <step> | claim N v|-        (N slots, vector maps written or not; 0 -: no claim)
#include <cstdio>
#include <vector>

#include "../mesh_navigation_amd/csrc/mnav_resident.h"

using mnav::Resident;

namespace {

constexpr double kOffset = 0.3;
const std::vector<uint32_t> kSeeds{ 10, 20, 30 }, kTargets{ 11, 21, 31 };
const std::vector<uint32_t> kAll{ 2, 0, 1 };     // device plan -> caller's index
const std::vector<uint32_t> kTwo{ 2, 0 };        // plan 1 was answered on the host

void show(const char* step, const Resident& r)
{
  const Resident::FinalizeClaim c = r.finalize_claim();
  std::printf("%s | claim %u %c\n", step, c.slots, c.slots && c.vecmaps ? 'v' : '-');
}

// a Dijkstra call that went through, the way dijkstra_impl drives the record: the claim is taken out before the outputs begin
Resident::FinalizeClaim call(Resident& r, const std::vector<uint32_t>& map, int engine, bool paths_only, bool vecmaps)
{
  r.record_dijkstra(3, kSeeds.data(), kTargets.data(), 1.0, kOffset);
  const Resident::FinalizeClaim held = r.take_finalize_claim();
  r.outputs_begin(Resident::kDijkstra, 3, map);
  r.commit_dijkstra(engine, (uint32_t)map.size(), paths_only, vecmaps);
  return held;
}

Resident claimed()
{
  Resident r;
  (void)call(r, kAll, 5, false, true);
  return r;
}

}  // namespace

int main()
{
  {
    Resident r;
    show("0 nothing yet", r);
  }
  // 1. what sets it: the commit of a finalized tile-batch call, and nothing else
  for (int engine : { 0, 1, 5, 6 }) {
    Resident r;
    (void)call(r, kAll, engine, false, true);
    char step[64];
    std::snprintf(step, sizeof step, "1 engine %d finalized vec", engine);
    show(step, r);
  }
  {
    Resident r;
    (void)call(r, kAll, 5, false, false);
    show("1 engine 5 finalized, no vector maps", r);
    (void)call(r, kAll, 5, true, false);
    show("1 engine 5 paths-only after it", r);
  }
  {
    Resident r;
    (void)call(r, kTwo, 5, false, true);
    show("1 engine 5, one plan answered on the host", r);
    (void)call(r, {}, 5, false, true);
    show("1 engine 5, every plan answered on the host", r);
  }
  // 2. the next call takes it out; it is that call's alone and comes back with that call's commit
  {
    Resident r = claimed();
    r.record_dijkstra(3, kSeeds.data(), kTargets.data(), 1.0, kOffset);
    show("2 next call recorded", r);
    const Resident::FinalizeClaim held = r.take_finalize_claim();
    std::printf("  taken %u %c\n", held.slots, held.vecmaps ? 'v' : '-');
    show("2 taken", r);
    r.outputs_begin(Resident::kDijkstra, 3, kAll);
    show("2 begun", r);
    r.commit_dijkstra(5, 3, false, false);
    show("2 committed without vector maps", r);
    const Resident::FinalizeClaim again = call(r, kAll, 5, false, true);
    std::printf("  the call after it held %u %c\n", again.slots, again.vecmaps ? 'v' : '-');
    show("2 committed with vector maps", r);
  }
  {
    Resident r = claimed();
    r.outputs_begin(Resident::kDijkstra, 3, kAll);                    // (a caller that forgot to take it: gone all the same)
    show("2 begun without taking", r);
  }
  {
    Resident r = claimed();
    r.record_dijkstra(3, kSeeds.data(), kTargets.data(), 1.0, kOffset);
    (void)r.take_finalize_claim();
    r.outputs_begin(Resident::kDijkstra, 3, kAll);
    show("2 begun, failed or cancelled", r);                          // (every error return of the plan calls: no commit)
  }
  // 3. everything after which something else may have written a slot
  {
    Resident r = claimed();
    r.outputs_begin(Resident::kCvp, 3, { 0, 1, 2 });
    show("3 cvp begun", r);
    r.commit_cvp(3);
    show("3 cvp committed", r);
  }
  {
    Resident r = claimed();
    r.repair_begin();
    show("3 repair begun", r);
    r.repair_commit(kTargets, kOffset, true);
    show("3 repair committed", r);
  }
  {
    Resident r = claimed();
    r.call_failed();
    show("3 call failed", r);
  }
  {
    Resident r = claimed();
    r.wave_took_slot0();
    show("3 inflation wave", r);
  }
  {
    Resident r = claimed();
    r.shard_took_slot0();
    show("3 sharded plan", r);
  }
  {
    Resident r = claimed();
    r.mesh_replaced();
    show("3 mesh replaced", r);
  }
  {
    Resident r = claimed();
    r.batch_state_freed();
    show("3 batch state freed", r);
  }
  // 4. what leaves it alone: the queries
  {
    Resident r = claimed();
    (void)r.slot(0); (void)r.available(0, 4); (void)r.may_keep(kOffset, true); (void)r.fields_resident();
    (void)r.replan_reason(3, kTargets, 100, 3, false);
    show("4 queries", r);
  }
  return 0;
}
