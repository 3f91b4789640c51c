"""CPU: the fleet schedule calls' C ABI as built -- the two symbols in the cross-compiled library, in the header and in
capi.SYMBOLS, the Python methods, the options, and the k_schedule_* kernels in the gfx950 code object inside libmnav.so (by
their names in its symbol table)."""
import ctypes as C
import os
import re
import subprocess

from mesh_navigation_amd import build as B
from mesh_navigation_amd import capi
from tests.test_follow_capi_cpu import llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_schedule_init", "k_schedule_probe", "k_schedule_claim", "k_schedule_decide", "k_schedule_commit", "k_schedule_next")
SYMBOLS = ("mnav_fleet_schedule", "mnav_schedule_stats")


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mnav.h")).read()
    names = set(re.findall(r"\b(mnav_[a-z_]+)\s*\(", hdr))
    L = C.CDLL(B.build_lib())
    for s in SYMBOLS:
        assert s in names and s in capi.SYMBOLS and hasattr(L, s), s
    for m in ("fleet_schedule", "schedule_stats"):
        assert hasattr(capi.MnavContext, m), m
    for name, value in (("NONE", 0), ("COMMITTED", 1), ("NO_SLOT", 2), ("OPEN", 3), ("SEED_FREE", 1)):
        assert getattr(capi, "SCHEDULE_" + name) == value and re.search(r"#define MNAV_SCHEDULE_%s %du\b" % (name, value), hdr), name
    opts = open(os.path.join(ROOT, "mesh_navigation_amd", "csrc", "mnav_options.h")).read()
    assert "X(schedule_chunk_rounds)" in opts and "X(schedule_clean_fill)" in opts


def test_the_kernels_are_in_the_gfx950_code_object(tmp_path):
    lib = B.build_lib()
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.check_call([llvm_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "stripped.so")])
    subprocess.check_call([llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    symbols = subprocess.check_output([llvm_tool("llvm-objdump"), "--syms", co], text=True).split()      # the symbol table only
    for k in KERNELS:
        hit = [s for s in symbols if re.fullmatch(r"_Z\w*" + k + r"E\w*", s)]                             # (no ".kd", no ".num_vgpr" ...)
        assert len(hit) == 1 and (hit[0] + ".kd") in symbols, (k, hit)       # the function and its kernel descriptor
