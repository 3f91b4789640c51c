"""When the tile-batch finalize pass may skip stores (csrc/mnav_resident.h, Resident::FinalizeClaim), on the CPU:
tests/finalize_claim_main.cpp is built alone with the host sanitizers (the header needs no HIP and no mnav_ctx), run as a child
process, and what the record says about the claim after every transition is compared with the table below.  Nothing is loaded
into this process.

The claim -- "the arrays of the first N plan slots hold what the last finalize pass of the tile-batch engine wrote, vector maps
included (v) or not (-)" -- is set by the commit of a finalized tile-batch call only, belongs to the call that takes it out, and
falls with every transition after which something else may have written a slot.  The same transitions, seen through the C ABI
on the device, are tests/test_gpu_tb_fin_keep.py."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLE = [
    "0 nothing yet | claim 0 -",
    # 1. only the tile-batch engine (5) has this finalize pass
    "1 engine 0 finalized vec | claim 0 -",
    "1 engine 1 finalized vec | claim 0 -",
    "1 engine 5 finalized vec | claim 3 v",
    "1 engine 6 finalized vec | claim 0 -",
    "1 engine 5 finalized, no vector maps | claim 3 -",
    "1 engine 5 paths-only after it | claim 0 -",                       # (it wrote no slot, but its outputs began: the rule has no exceptions)
    "1 engine 5, one plan answered on the host | claim 2 v",            # device plans are slots 0 and 1
    "1 engine 5, every plan answered on the host | claim 0 -",
    # 2. the next call
    "2 next call recorded | claim 3 v",                                 # (recording changes no slot)
    "  taken 3 v",
    "2 taken | claim 0 -",
    "2 begun | claim 0 -",
    "2 committed without vector maps | claim 3 -",
    "  the call after it held 3 -",
    "2 committed with vector maps | claim 3 v",
    "2 begun without taking | claim 0 -",
    "2 begun, failed or cancelled | claim 0 -",
    # 3. other writers of the slots
    "3 cvp begun | claim 0 -",
    "3 cvp committed | claim 0 -",
    "3 repair begun | claim 0 -",
    "3 repair committed | claim 0 -",                                   # (a repair's passes name the slots in their own order)
    "3 call failed | claim 0 -",
    "3 inflation wave | claim 0 -",
    "3 sharded plan | claim 0 -",
    "3 mesh replaced | claim 0 -",
    "3 batch state freed | claim 0 -",
    "4 queries | claim 3 v",
]


def test_the_claim_stands_exactly_when_the_slots_are_the_last_pass_s(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the stand-alone claim program"
    exe = str(tmp_path / "finalize_claim")
    # the runtimes are linked into the program: it needs nothing preloaded
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "finalize_claim_main.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and not run.stderr, run.stderr
    got = run.stdout.splitlines()
    for k, want in enumerate(TABLE):
        assert k < len(got) and got[k] == want, (k, got[k] if k < len(got) else None, want)
    assert len(got) == len(TABLE), got[len(TABLE):]
