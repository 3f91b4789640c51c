// mnav_resident.h -- the record of what the last plan call left on the device.  Host logic only: plain
// C++17, no HIP, no mnav_ctx; tests/resident_record_main.cpp compiles it alone.
//
// Everything that works on resident outputs (the follower, rollouts, the replans, the fleet calls, mnav_device_output and the
// downloads) asks the same questions: which plans of the last call reached the device and in which slot, which of their
// outputs are there, whether the distances can be rewound, whether something took slot 0 since.  The answers live here and
// nowhere else.  State changes through the transitions only, readers go through the queries only.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

namespace mnav {

class Resident {
 public:
  static constexpr uint32_t kNone = 0xFFFFFFFFu;                     // a plan that never reached the device
  enum Kind : uint8_t { kNoCall, kDijkstra, kCvp, kSharded };        // the call that owns the outputs
  // "The arrays of the first `slots` plan slots hold what the tile-batch engine's last finalize pass wrote, vector maps included
  // or not": what lets the next such pass skip the stores of a (tile, plan) whose unreached pattern it wrote last time
  // (mnav_tb_finalize.h).  It stands from the commit of a fresh tile-batch call that was finalized until the next transition
  // after which something else may have written a slot -- every one but the commits.
  struct FinalizeClaim { uint32_t slots = 0; bool vecmaps = false; };

  // -- transitions ----------------------------------------------------------------------------------------------------
  // A Dijkstra call is recorded (what a replan needs of it, in the caller's order); its fields count once it has committed.
  // The outputs still on the device stay described as they are until outputs_begin.
  void record_dijkstra(uint32_t n, const uint32_t* seeds, const uint32_t* targets, double cost_limit, double offset)
  {
    const std::vector<uint32_t> s(seeds, seeds + n), t(targets, targets + n);   // (the caller's arrays may be the record's own)
    seeds_ = s; targets_ = t; cost_limit_ = cost_limit; offset_ = offset;
    have_call_ = true; rewindable_ = false; partial_ = false;
  }
  // The outputs of a call of n plans begin: those of the previous call are gone.  map: device plan -> caller's index.
  void outputs_begin(Kind kind, uint32_t n, const std::vector<uint32_t>& map)
  {
    fin_claim_ = FinalizeClaim{};                                     // (the starting call took it out first: take_finalize_claim)
    kind_ = kind; hidden_ = false; live_ = 0;
    slot_.assign(n, kNone);
    for (size_t k = 0; k < map.size(); ++k) slot_[map[k]] = (uint32_t)k;
    finalized_ = vec_ = rewindable_ = partial_ = false;
  }
  // The Dijkstra call went through with `live` device plans (0: every plan was answered on the host).
  void commit_dijkstra(int engine, uint32_t live, bool paths_only, bool vecmaps)
  {
    if (live) {
      live_ = live; finalized_ = !paths_only; vec_ = vecmaps;
      rewindable_ = leaves_rewindable_field(engine, paths_only);
      if (engine == 5 && !paths_only) { fin_claim_.slots = live; fin_claim_.vecmaps = vecmaps; }   // (a fresh call: device plan k is slot k)
    }
    slot0_taken_ = false;
    partial_ = live != slot_.size();
    note_robots();
  }
  // slots[k].dist is a field a replan can rewind: below the cut every value is final after the tile rounds (0) and the
  // asynchronous tiles (6), finalized or not, and after the tile-batch engine's (5) finalize pass; the band steps (1) keep
  // other values
  static bool leaves_rewindable_field(int engine, bool paths_only) { return engine == 0 || engine == 6 || (engine == 5 && !paths_only); }
  // The CVP call's engine went through: potentials, predecessors and vector maps of `live` plans.
  void commit_cvp(uint32_t live) { live_ = live; finalized_ = vec_ = true; }
  // A repair starts to change the recorded fields (an inflation wave in between took slot 0's bookkeeping, not its dist: the
  // map is the recorded call's again).
  void repair_begin() { kind_ = kDijkstra; hidden_ = false; live_ = 0; rewindable_ = false; fin_claim_ = FinalizeClaim{}; }
  // The repair went through, finalize pass included: the record follows the new robot vertices and offset.
  void repair_commit(const std::vector<uint32_t>& targets, double offset, bool vecmaps)
  {
    targets_ = targets; offset_ = offset;
    live_ = (uint32_t)slot_.size(); finalized_ = true; vec_ = vecmaps; rewindable_ = true; slot0_taken_ = false;
    note_robots();
  }
  // The call failed or was cancelled: nothing is handed out, nothing can be rewound (the fields may be half rewound).
  void call_failed() { live_ = 0; rewindable_ = false; fin_claim_ = FinalizeClaim{}; }
  // An inflation wave worked in plan slot 0: the outputs are hidden (the wave took slot 0's predecessors, keys and lists; a
  // replan re-derives them, and keeps no plan in slot 0 as it is).  The recorded call and its map stay for the replan.
  void wave_took_slot0() { hidden_ = true; slot0_taken_ = true; fin_claim_ = FinalizeClaim{}; }
  // Slot 0 and the result records were taken over by a sharded plan: nothing a replan can rewind.
  void shard_took_slot0()
  {
    kind_ = kSharded; hidden_ = false; live_ = 0; slot_.clear(); fin_claim_ = FinalizeClaim{};
    finalized_ = vec_ = rewindable_ = partial_ = false;
  }
  // The mesh was replaced: the recorded seeds are the old mesh's.  (As found: the map and the live count stay -- the slots
  // themselves are gone, so nothing is handed out, but the robot-side calls still see the old plan count.)
  void mesh_replaced() { have_call_ = rewindable_ = partial_ = false; fin_claim_ = FinalizeClaim{}; }
  // The tile-batch engine's batch state was freed (a larger batch, a new mesh): the map the claim speaks of is gone.
  void batch_state_freed() { fin_claim_ = FinalizeClaim{}; }
  // The call that starts takes the claim out, before its outputs_begin: it alone may use it, and only if it turns out to be a
  // fresh tile-batch call; the claim is gone until that call commits.
  FinalizeClaim take_finalize_claim() { const FinalizeClaim c = fin_claim_; fin_claim_ = FinalizeClaim{}; return c; }

  // -- queries --------------------------------------------------------------------------------------------------------
  Kind kind() const { return kind_; }
  // As found: before the first plan call and after a sharded plan the readers answer as after a Dijkstra call without outputs.
  bool dijkstra_family() const { return kind_ != kCvp; }
  uint32_t live() const { return live_; }                             // device plans that hold outputs (0: call in progress, failed, cancelled)
  // the plans the robot-side calls see.  As found: 1 after an inflation wave, whatever the batch was
  size_t plans() const { return hidden_ ? 1 : slot_.size(); }
  // device slot of the caller's plan i; kNone: not a plan of the last call, never reached the device, or hidden
  uint32_t slot(uint32_t i) const { return (hidden_ || i >= slot_.size()) ? kNone : slot_[i]; }
  // As found (popped potential, vector_at after a paths-only tile-batch call): an index beyond the map is taken as a device slot.
  uint32_t slot_or_raw(uint32_t i) const { return i < plans() ? slot(i) : i; }
  // whether output `what` (0 dist, 1 pred, 2 direction, 3 cut face, 4 vector map) of the caller's plan i can be handed out.  A
  // paths-only Dijkstra call finalized nothing (values beyond goal_dist are engine-tentative, predecessors exist along the path
  // only); a Dijkstra call that was not asked for vector maps must not hand out an earlier call's
  bool available(uint32_t i, int what) const
  {
    if (slot(i) >= live_) return false;
    switch (what) {
      case 0: case 1: return finalized_;
      case 2: case 3: return true;
      case 4: return vec_;
      default: return false;
    }
  }
  bool paths_only() const { return dijkstra_family() && !finalized_; }
  uint32_t robot_vertex(uint32_t device_slot) const { return robot_[device_slot]; }   // Dijkstra, device_slot < live()

  // the recorded Dijkstra call
  bool has_recorded_call() const { return have_call_; }
  const std::vector<uint32_t>& seeds() const { return seeds_; }
  const std::vector<uint32_t>& targets() const { return targets_; }
  double cost_limit() const { return cost_limit_; }
  double offset() const { return offset_; }
  uint32_t recorded_slot(uint32_t i) const { return slot_[i]; }        // the map of the recorded call, hidden or not (i < seeds().size())
  bool slot0_lost() const { return slot0_taken_; }
  // slots[k].dist holds the reference's values below the cut (not after the band steps, a paths-only tile-batch call, a
  // failed or cancelled call, a half-rewound replan)
  bool rewindable() const { return rewindable_; }
  // the outputs on the device are the recorded call's.  (As found: a single plan that never reached the device stays
  // "resident" through an inflation wave -- there is nothing the wave could have taken.)
  bool fields_resident() const
  {
    if (!have_call_ || !dijkstra_family() || slot_.size() != seeds_.size() || targets_.size() != seeds_.size()) return false;
    return !hidden_ || (slot_.size() == 1 && slot_[0] == kNone);
  }
  // why a replan of n plans towards `targets` plans the whole call afresh: 0 (it does not: repair), 1 (no rewindable fields
  // of that call), 2 (everything changed), 3 (a plan of the call never reached the device, or would not with its new target)
  uint32_t replan_reason(uint32_t n, const std::vector<uint32_t>& targets, uint32_t V, size_t device_slots, bool everything_changed) const
  {
    if (partial_ && dijkstra_family()) return 3;                      // (none of them reached it: no field either)
    if (!rewindable_ || !dijkstra_family() || live_ != n || slot_.size() != n || device_slots < n) return 1;
    if (everything_changed) return 2;
    for (uint32_t i = 0; i < n; ++i)
      if (slot_[i] >= n || targets[i] >= V || targets[i] == seeds_[i]) return 3;
    return 0;
  }
  // the per-plan replan keeps a plan as it is only when its field went through a finalize pass, its vector map (if one is
  // wanted) is resident and the offset has the recorded bits
  bool may_keep(double offset, bool want_vecmaps) const
  {
    return finalized_ && (!want_vecmaps || vec_) && memcmp(&offset, &offset_, sizeof(double)) == 0;
  }
  FinalizeClaim finalize_claim() const { return fin_claim_; }

 private:
  void note_robots()                                                  // robot vertex per device slot, for the popped potential
  {
    robot_.assign(live_, kNone);
    for (size_t i = 0; i < slot_.size() && i < targets_.size(); ++i) if (slot_[i] < live_) robot_[slot_[i]] = targets_[i];
  }

  Kind kind_ = kNoCall;
  std::vector<uint32_t> slot_;       // caller's plan index -> device slot of the call that owns the outputs (kNone: never ran)
  bool hidden_ = false;              // an inflation wave took slot 0 since: nothing is handed out, the robot-side calls see one plan
  uint32_t live_ = 0;
  bool finalized_ = false;           // dist and pred went through a finalize pass (Dijkstra: not a paths-only call) or are a CVP call's
  bool vec_ = false;                 // vector maps were written
  bool rewindable_ = false;
  std::vector<uint32_t> robot_;
  // the recorded Dijkstra call.  As found: it survives a CVP call and a sharded plan (a replan then answers with reason 1)
  std::vector<uint32_t> seeds_, targets_;
  double cost_limit_ = 1.0, offset_ = 0.0;
  bool have_call_ = false;
  bool partial_ = false;             // the call went through, but a plan of it never reached the device (rejected ids, seed == target)
  bool slot0_taken_ = false;
  FinalizeClaim fin_claim_;
};

}  // namespace mnav
