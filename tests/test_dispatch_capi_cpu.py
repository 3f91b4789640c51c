"""CPU: the dispatch calls' C ABI as built -- the three symbols in the cross-compiled library, in the header and in
capi.SYMBOLS, the Python methods, the options, and the k_dispatch_* kernels in the gfx950 code object inside libmnav.so (by
their names in its symbol table)."""
import ctypes as C
import os
import re
import subprocess

from mesh_navigation_amd import build as B
from mesh_navigation_amd import capi
from tests.test_follow_capi_cpu import llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_dispatch_costs", "k_dispatch_resolve", "k_dispatch_nearest", "k_dispatch_quantise", "k_dispatch_bid", "k_dispatch_award", "k_dispatch_tail",
           "k_dispatch_result")


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mnav.h")).read()
    names = set(re.findall(r"\b(mnav_[a-z_]+)\s*\(", hdr))
    L = C.CDLL(B.build_lib())
    for s in ("mnav_fleet_costs", "mnav_fleet_assign", "mnav_dispatch_stats"):
        assert s in names and s in capi.SYMBOLS and hasattr(L, s), s
    for m in ("fleet_costs", "fleet_assign", "dispatch_stats"):
        assert hasattr(capi.MnavContext, m), m
    opts = open(os.path.join(ROOT, "mesh_navigation_amd", "csrc", "mnav_options.h")).read()
    for o in ("dispatch_max_mb", "dispatch_max_rounds", "dispatch_tail_bidders"):
        assert "X(%s)" % o in opts, o


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
