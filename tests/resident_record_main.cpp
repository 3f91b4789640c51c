// Walks the record of the resident outputs (csrc/mnav_resident.h) through the sequences of calls the library makes and prints
// what its queries answer after every step, one line per step.  tests/test_resident_record.py builds this file alone, with
// the host sanitizers, runs it and compares the lines with its table.
//
//   <step> | slots a,b,c | out dpv,dpv,dpv | plans N live L | resident R rewind W | reason X | keep same other vec
//
// slots: device slot per caller plan (- = none); out: which of dist, pred, vector map can be handed out per caller plan;
// plans: what the robot-side calls see; reason: of a replan towards the recorded targets (- = no recorded call: refused);
// keep: may_keep for the recorded offset, for another one, and for the recorded one with vector maps wanted.
#include <cstdio>
#include <string>
#include <vector>

#include "../mesh_navigation_amd/csrc/mnav_resident.h"

using mnav::Resident;

namespace {

constexpr uint32_t kV = 100;        // vertices of the mesh
constexpr size_t kDeviceSlots = 3;  // what ensure_slots has allocated
constexpr double kOffset = 0.3;

void show(const char* step, const Resident& r, uint32_t n)
{
  std::string slots, out;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t s = r.slot(i);
    slots += (i ? "," : "") + (s == Resident::kNone ? std::string("-") : std::to_string(s));
    out += i ? "," : "";
    out += r.available(i, 0) ? 'd' : '-';
    out += r.available(i, 1) ? 'p' : '-';
    out += r.available(i, 4) ? 'v' : '-';
  }
  std::string reason = "-";
  if (r.has_recorded_call()) reason = std::to_string(r.replan_reason((uint32_t)r.seeds().size(), r.targets(), kV, kDeviceSlots, false));
  std::printf("%s | slots %s | out %s | plans %zu live %u | resident %d rewind %d | reason %s | keep %d %d %d\n", step, slots.c_str(), out.c_str(), r.plans(),
              r.live(), r.fields_resident() ? 1 : 0, r.rewindable() ? 1 : 0, reason.c_str(), r.may_keep(r.offset(), false) ? 1 : 0,
              r.may_keep(0.5, false) ? 1 : 0, r.may_keep(r.offset(), true) ? 1 : 0);
}

const std::vector<uint32_t> kSeeds{ 10, 20, 30 }, kTargets{ 11, 21, 31 };
const std::vector<uint32_t> kAll{ 2, 0, 1 };     // device plan -> caller's index, as dijkstra_order left it
const std::vector<uint32_t> kTwo{ 2, 0 };        // plan 1 was answered on the host

// record, begin, commit: a Dijkstra call that went through
Resident dijkstra(const std::vector<uint32_t>& targets, const std::vector<uint32_t>& map, int engine, bool paths_only, bool vecmaps)
{
  Resident r;
  r.record_dijkstra(3, kSeeds.data(), targets.data(), 1.0, kOffset);
  r.outputs_begin(Resident::kDijkstra, 3, map);
  r.commit_dijkstra(engine, (uint32_t)map.size(), paths_only, vecmaps);
  return r;
}

}  // namespace

int main()
{
  {
    Resident r;
    show("0 nothing yet", r, 3);
  }
  // 1. a Dijkstra call on each engine
  {
    Resident r;
    r.record_dijkstra(3, kSeeds.data(), kTargets.data(), 1.0, kOffset);
    show("1 recorded", r, 3);
    r.outputs_begin(Resident::kDijkstra, 3, kAll);
    show("1 begun", r, 3);
    r.commit_dijkstra(0, 3, false, true);
    show("1 engine 0 finalized vec", r, 4);
    std::printf("  robot vertices %u %u %u offset %g plans recorded %zu\n", r.robot_vertex(0), r.robot_vertex(1), r.robot_vertex(2), r.offset(), r.seeds().size());
  }
  show("1 engine 0 paths-only", dijkstra(kTargets, kAll, 0, true, false), 3);
  show("1 engine 5 finalized", dijkstra(kTargets, kAll, 5, false, false), 3);
  show("1 engine 5 paths-only", dijkstra(kTargets, kAll, 5, true, false), 3);
  show("1 engine 6 paths-only", dijkstra(kTargets, kAll, 6, true, false), 3);
  show("1 engine 1", dijkstra(kTargets, kAll, 1, false, true), 3);
  // 2. plans that never reached the device
  show("2 one rejected", dijkstra({ 11, 20, 31 }, kTwo, 0, false, true), 3);
  show("2 all rejected", dijkstra(kSeeds, {}, 0, false, true), 3);
  // 3. the call fails after its outputs began (every error return of the plan calls; the replans say call_failed on top)
  {
    Resident r = dijkstra(kTargets, kAll, 0, false, true);
    r.record_dijkstra(3, kSeeds.data(), kTargets.data(), 1.0, kOffset);
    r.outputs_begin(Resident::kDijkstra, 3, kAll);
    show("3 begun, failed", r, 3);
  }
  // 4. an inflation wave takes slot 0, a repair brings the outputs back
  {
    Resident r = dijkstra(kTargets, kAll, 0, false, true);
    r.wave_took_slot0();
    show("4 wave", r, 3);
    std::printf("  slot 0 taken %d; raw index 1 -> %u, index 0 -> %s\n", r.slot0_lost() ? 1 : 0, r.slot_or_raw(1), r.slot_or_raw(0) == Resident::kNone ? "-" : "?");
    r.repair_begin();
    show("4 repair begun", r, 3);
    r.repair_commit(kTargets, kOffset, true);
    show("4 repair committed", r, 3);
    std::printf("  slot 0 taken %d\n", r.slot0_lost() ? 1 : 0);
  }
  // 5. a CVP call takes the outputs; the recorded Dijkstra call survives
  for (uint32_t n : { 2u, 3u }) {
    Resident r = dijkstra(kTargets, kAll, 0, false, true);
    std::vector<uint32_t> map(n);
    for (uint32_t k = 0; k < n; ++k) map[k] = k;
    r.outputs_begin(Resident::kCvp, n, map);
    show(n == 2 ? "5 cvp of 2 begun" : "5 cvp of 3 begun", r, 3);
    r.commit_cvp(n);
    show(n == 2 ? "5 cvp of 2 committed" : "5 cvp of 3 committed", r, 3);
  }
  // 6. a sharded plan takes slot 0
  {
    Resident r = dijkstra(kTargets, kAll, 0, false, true);
    r.shard_took_slot0();
    show("6 sharded", r, 3);
  }
  // 7. a repair fails
  {
    Resident r = dijkstra(kTargets, kAll, 0, false, true);
    r.repair_begin();
    r.call_failed();
    show("7 repair failed", r, 3);
  }
  // 8. a repair towards new targets and another offset
  {
    Resident r = dijkstra(kTargets, kAll, 0, false, false);
    r.repair_begin();
    r.repair_commit({ 12, 22, 32 }, 0.5, true);
    show("8 repaired to new targets", r, 3);
    std::printf("  targets %u %u %u robot vertices %u %u %u offset %g keep(0.3) %d\n", r.targets()[0], r.targets()[1], r.targets()[2], r.robot_vertex(0), r.robot_vertex(1),
                r.robot_vertex(2), r.offset(), r.may_keep(kOffset, false) ? 1 : 0);
    const double neg_zero = -0.0;
    r.repair_begin();
    r.repair_commit({ 12, 22, 32 }, 0.0, true);
    std::printf("  offset +0: keep(+0) %d keep(-0) %d\n", r.may_keep(0.0, true) ? 1 : 0, r.may_keep(neg_zero, true) ? 1 : 0);
    std::printf("  a new target on its seed: reason %u; beyond the mesh: reason %u; everything changed: reason %u; fewer device slots: reason %u\n",
                r.replan_reason(3, { 12, 20, 32 }, kV, kDeviceSlots, false), r.replan_reason(3, { 12, 22, kV }, kV, kDeviceSlots, false),
                r.replan_reason(3, r.targets(), kV, kDeviceSlots, true), r.replan_reason(3, r.targets(), kV, 2, false));
  }
  // 9. the mesh is replaced
  {
    Resident r = dijkstra(kTargets, kAll, 0, false, true);
    r.mesh_replaced();
    show("9 mesh replaced", r, 3);
  }
  return 0;
}
