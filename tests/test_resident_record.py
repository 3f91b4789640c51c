"""The record of the resident outputs (csrc/mnav_resident.h) on the CPU: tests/resident_record_main.cpp is built alone with the
host sanitizers (the header needs no HIP and no mnav_ctx), run as a child process, and what its queries answer after every
transition is compared with the table below.  Nothing is loaded into this process.

The table was derived from the code BEFORE the record existed (commit b842d8c), where about fifteen members of mnav_ctx held
these answers; next to each row stands the place in that code it rests on (mnav.hip unless another file is named).  The same
rows, seen through the C ABI on the device, are tests/test_gpu_resident_record.py, which passed against that commit's library.

One line per step:
  <step> | slots a,b,c | out dpv,.. | plans N live L | resident R rewind W | reason X | keep same other vec
slots: device slot per caller plan (- none); out: dist, pred, vector map that can be handed out per caller plan; plans: what
the follower and the fleet walks see; live: device plans with outputs; resident: the outputs are the recorded Dijkstra call's
(mnav_fleet_capi.h:66); rewind: its distances can be rewound (rp.usable); reason: of a replan towards the recorded targets (-:
refused, no recorded call); keep: the per-plan replan may keep a plan, for the recorded offset, another one, and with vector
maps wanted."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLE = [
    # before any call: last_planner = 0 = Dijkstra, caller_slot empty, rp.have_call false (replan refused: mnav_replan_capi.h:240)
    ("0 nothing yet | slots -,-,- | out ---,---,--- | plans 0 live 0 | resident 0 rewind 0 | reason - | keep 0 0 0", "mnav_ctx defaults :153, :256, :286"),
    # 1. a Dijkstra call.  Recorded: seeds, targets, have_call, usable = partial = false (:1635-1638); the previous map stays until :1671
    ("1 recorded | slots -,-,- | out ---,---,--- | plans 0 live 0 | resident 0 rewind 0 | reason 1 | keep 0 0 0", ":1635-1638; reason: !usable mnav_replan_capi.h:252"),
    # begun: caller_slot = inverse of the device order, last_n = 0 (:1671-1679).  (resident: what a call that fails here leaves when
    # the call before it had the same map -- row 3; with another map the old code said 0, mnav_fleet_capi.h:66.)
    ("1 begun | slots 1,2,0 | out ---,---,--- | plans 3 live 0 | resident 1 rewind 0 | reason 1 | keep 0 0 0", ":1671-1679; :1950 last_n == 0"),
    ("1 engine 0 finalized vec | slots 1,2,0,- | out dpv,dpv,dpv,--- | plans 3 live 3 | resident 1 rewind 1 | reason 0 | keep 1 0 1", ":1685, :1690-1696; plan 3: :1948"),
    ("  robot vertices 31 11 21 offset 0.3 plans recorded 3", ":1678-1679 last_target[k] = in[k].target[0]"),
    ("1 engine 0 paths-only | slots 1,2,0 | out ---,---,--- | plans 3 live 3 | resident 1 rewind 1 | reason 0 | keep 0 0 0", ":1954-1960 lazy; :1690 engine 0 rewindable; :1691 not finalized"),
    ("1 engine 5 finalized | slots 1,2,0 | out dp-,dp-,dp- | plans 3 live 3 | resident 1 rewind 1 | reason 0 | keep 1 0 0", ":1690 engine 5 && !lazy; :1960 no vector maps asked; mnav_replan_each_capi.h:91"),
    ("1 engine 5 paths-only | slots 1,2,0 | out ---,---,--- | plans 3 live 3 | resident 1 rewind 0 | reason 1 | keep 0 0 0", ":1690 engine 5 && lazy: not rewindable"),
    ("1 engine 6 paths-only | slots 1,2,0 | out ---,---,--- | plans 3 live 3 | resident 1 rewind 1 | reason 0 | keep 0 0 0", ":1690 engine 6"),
    ("1 engine 1 | slots 1,2,0 | out dpv,dpv,dpv | plans 3 live 3 | resident 1 rewind 0 | reason 1 | keep 1 0 1", ":1686 never paths-only; :1690 never rewindable"),
    # 2. plans answered on the host
    ("2 one rejected | slots 1,-,0 | out dpv,---,dpv | plans 3 live 2 | resident 1 rewind 1 | reason 3 | keep 1 0 1", ":1696 partial; mnav_replan_capi.h:251"),
    ("2 all rejected | slots -,-,- | out ---,---,--- | plans 3 live 0 | resident 1 rewind 0 | reason 3 | keep 0 0 0", ":1680 m == 0 skips :1685-1692; :1696"),
    # 3. every error return between :1681 and :1687
    ("3 begun, failed | slots 1,2,0 | out ---,---,--- | plans 3 live 0 | resident 1 rewind 0 | reason 1 | keep 0 0 0", ":1677 last_n = 0, :1637 usable = false; mnav_fleet_capi.h:66 (same map), :84"),
    # 4. the inflation wave: caller_slot.assign(1, kNone), rp.slot0_taken (:1134-1135); rp.caller_slot, rp.usable and last_n stay
    ("4 wave | slots -,-,- | out ---,---,--- | plans 1 live 3 | resident 0 rewind 1 | reason 0 | keep 1 0 1", ":1134-1135; mnav_fleet_capi.h:66 caller_slot != rp.caller_slot; mnav_replan_capi.h:252"),
    ("  slot 0 taken 1; raw index 1 -> 1, index 0 -> -", "mnav_replan_each_capi.h:94; :1978, :2013 `if (slot < caller_slot.size())`"),
    ("4 repair begun | slots 1,2,0 | out ---,---,--- | plans 3 live 0 | resident 1 rewind 0 | reason 1 | keep 1 0 1", "mnav_replan_capi.h:170-174"),
    ("4 repair committed | slots 1,2,0 | out dpv,dpv,dpv | plans 3 live 3 | resident 1 rewind 1 | reason 0 | keep 1 0 1", "mnav_replan_capi.h:198, :213-214"),
    ("  slot 0 taken 0", "mnav_replan_capi.h:214"),
    # 5. a CVP call: its own map and count (:1773-1779, :1793), always dist, pred and vector maps (:1954, :1960); rp.have_call stays
    ("5 cvp of 2 begun | slots 0,1,- | out ---,---,--- | plans 2 live 0 | resident 0 rewind 0 | reason 1 | keep 0 0 0", ":1773-1779"),
    ("5 cvp of 2 committed | slots 0,1,- | out dpv,dpv,--- | plans 2 live 2 | resident 0 rewind 0 | reason 1 | keep 1 0 1", ":1793; mnav_fleet_capi.h:66 last_planner; mnav_replan_capi.h:252"),
    ("5 cvp of 3 begun | slots 0,1,2 | out ---,---,--- | plans 3 live 0 | resident 0 rewind 0 | reason 1 | keep 0 0 0", ":1773-1779"),
    ("5 cvp of 3 committed | slots 0,1,2 | out dpv,dpv,dpv | plans 3 live 3 | resident 0 rewind 0 | reason 1 | keep 1 0 1", "the same with last_n == n: mnav_replan_capi.h:252 !usable"),
    # 6. mnav_shard_begin: caller_slot.clear(), last_n = 0, usable = partial = false
    ("6 sharded | slots -,-,- | out ---,---,--- | plans 0 live 0 | resident 0 rewind 0 | reason 1 | keep 0 0 0", "mnav_shard_capi.h:181-184"),
    # 7. / 8. repairs
    ("7 repair failed | slots 1,2,0 | out ---,---,--- | plans 3 live 0 | resident 1 rewind 0 | reason 1 | keep 1 0 1", "mnav_replan_capi.h:172, :267-271"),
    ("8 repaired to new targets | slots 1,2,0 | out dpv,dpv,dpv | plans 3 live 3 | resident 1 rewind 1 | reason 0 | keep 1 1 1", "mnav_replan_capi.h:213-214 (the other offset IS the recorded one now)"),
    ("  targets 12 22 32 robot vertices 32 12 22 offset 0.5 keep(0.3) 0", "mnav_replan_capi.h:173, :213"),
    ("  offset +0: keep(+0) 1 keep(-0) 0", "mnav_replan_each_capi.h:91 memcmp"),
    ("  a new target on its seed: reason 3; beyond the mesh: reason 3; everything changed: reason 2; fewer device slots: reason 1", "mnav_replan_capi.h:252-256"),
    # 9. mnav_upload_mesh: have_call = usable = partial = false; map and count stay, the slots themselves are gone (slots.clear(), :710)
    ("9 mesh replaced | slots 1,2,0 | out dpv,dpv,dpv | plans 3 live 3 | resident 0 rewind 0 | reason - | keep 1 0 1", ":711"),
]


def test_the_record_answers_as_the_members_it_replaced(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the stand-alone record program"
    exe = str(tmp_path / "resident_record")
    # the runtimes are linked into the program: it needs nothing preloaded and does not care what else the loader brings
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "resident_record_main.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and not run.stderr, run.stderr
    got = run.stdout.splitlines()
    for k, (want, rests_on) in enumerate(TABLE):
        assert k < len(got) and got[k] == want, (k, rests_on, got[k] if k < len(got) else None, want)
    assert len(got) == len(TABLE), got[len(TABLE):]


def test_the_header_stands_alone():
    """plain C++17 over <vector>, <cstdint> and <cstring>: no HIP, nothing of the library"""
    src = open(os.path.join(ROOT, "mesh_navigation_amd", "csrc", "mnav_resident.h")).read()
    includes = [line.split()[1] for line in src.splitlines() if line.startswith("#include")]
    assert sorted(includes) == ["<cstdint>", "<cstring>", "<vector>"], includes
