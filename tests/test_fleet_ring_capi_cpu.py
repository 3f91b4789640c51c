"""CPU: the C ABI of the wait-for analysis as built -- the two symbols in the cross-compiled library, in the header and in
capi.SYMBOLS, the ctypes layout of mnav_ring_config and the values of MNAV_RING_* / MNAV_WAIT_* against a compiled probe of
include/mnav.h, the ring group behind every argument of mnav_fleet_rollout_yield, and the four k_ring_* kernels in the gfx950
code object inside libmnav.so (by their names in its symbol table), beside the yielding rollout's kernels, which a call without
a ring config still runs."""
import ctypes as C
import os
import re
import shutil
import subprocess

from mesh_navigation_amd import build as B
from mesh_navigation_amd import capi
from tests import ring_model as RG
from tests.test_fleet_yield_capi_cpu import KERNELS as YIELD_KERNELS
from tests.test_follow_capi_cpu import llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_ring_pair", "k_ring_double", "k_ring_close", "k_ring_rows")


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mnav.h")).read()
    names = set(re.findall(r"\b(mnav_[a-z_]+)\s*\(", hdr))
    L = C.CDLL(B.build_lib())
    for s in ("mnav_fleet_rollout_rings", "mnav_fleet_ring_stats"):
        assert s in names and s in capi.SYMBOLS and hasattr(L, s), s
    assert "typedef struct mnav_ring_config" in hdr
    assert hasattr(capi.MnavContext, "fleet_rollout_rings") and hasattr(capi.MnavContext, "fleet_ring_stats")
    assert issubclass(capi.FleetRingOut, capi.FleetYieldOut)

    # the ring group follows every argument of mnav_fleet_rollout_yield, in its order
    def args(name):
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr).group(1)
        return [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]
    yld, ring = args("mnav_fleet_rollout_yield"), args("mnav_fleet_rollout_rings")
    assert ring[: len(yld)] == yld
    assert ring[len(yld):] == ["rings", "wait_class_out", "wait_anchor_out", "ring_checks_out", "first_ring_tick_out", "parked_checks_out", "released_checks_out"]
    assert [a[: -len("_out")] for a in ring[len(yld) + 1:]] == list(capi.RING_OUTPUTS)
    assert len(capi.load().mnav_fleet_rollout_rings.argtypes) == len(ring) and len(capi.load().mnav_fleet_ring_stats.argtypes) == len(args("mnav_fleet_ring_stats"))
    # the rule stands in the header in full: the terms a model is written from
    for term in ("BLOCKER", "CHAIN", "ROOT", "RING", "LEADER", "at least three", "RELEASE", "hold0"):
        assert term in hdr, term


def test_config_layout_and_values_match_the_header(tmp_path):
    values = ["MNAV_RING_RELEASE", "MNAV_WAIT_FREE", "MNAV_WAIT_QUEUED", "MNAV_WAIT_PARKED", "MNAV_WAIT_RING_TAIL", "MNAV_WAIT_RING_MEMBER"]
    probe = '#include <stddef.h>\n#include <stdio.h>\n#include "mnav.h"\nint main(void) { mnav_ring_config d; printf("%zu %zu %zu", sizeof(mnav_ring_config), ' \
            'offsetof(mnav_ring_config, flags), sizeof(d.flags)); ' + " ".join('printf(" %%u", (unsigned)%s);' % v for v in values) + " return 0; }\n"
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(probe)
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("g++")
    assert cc, "a C compiler is needed for the layout probe"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == C.sizeof(capi.RingConfig) == 4 and out[1] == capi.RingConfig.flags.offset == 0 and out[2] == capi.RingConfig.flags.size == 4
    assert [n for n, _ in capi.RingConfig._fields_] == ["flags"]
    assert out[3:] == [capi.RING_RELEASE, capi.WAIT_FREE, capi.WAIT_QUEUED, capi.WAIT_PARKED, capi.WAIT_RING_TAIL, capi.WAIT_RING_MEMBER] == [1, 0, 1, 2, 3, 4]
    assert out[3:] == [RG.RELEASE, RG.FREE, RG.QUEUED, RG.PARKED, RG.RING_TAIL, RG.RING_MEMBER]          # the model's
    assert (capi.RingConfig().flags, capi.RingConfig(flags=1).flags) == (0, 1)


def test_the_kernels_are_in_the_gfx950_code_object(tmp_path):
    lib = B.build_lib()
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.check_call([llvm_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "stripped.so")])
    subprocess.check_call([llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    symbols = subprocess.check_output([llvm_tool("llvm-objdump"), "--syms", co], text=True).split()      # the symbol table only
    for k in KERNELS + YIELD_KERNELS:
        hit = [s for s in symbols if re.fullmatch(r"_Z\w*" + k + r"\w*", s)]                              # (no ".kd", no ".num_vgpr" ...)
        assert len(hit) == 1 and (hit[0] + ".kd") in symbols, (k, hit)       # the function and its kernel descriptor
