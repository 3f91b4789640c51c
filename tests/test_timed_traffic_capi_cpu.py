"""CPU: the timed fleet traffic calls' C ABI as built -- the five symbols in the cross-compiled library, in the header and
in capi.SYMBOLS, the Python methods, the option, and the k_timed_* kernels in the gfx950 code object inside libmnav.so (by
their names in its symbol table)."""
import ctypes as C
import os
import re
import subprocess

from mesh_navigation_amd import build as B
from mesh_navigation_amd import capi
from tests.test_follow_capi_cpu import llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_timed_add", "k_timed_peak", "k_timed_report")
SYMBOLS = ("mnav_fleet_timed_traffic", "mnav_timed_traffic_download", "mnav_timed_traffic_stats", "mnav_layer_timed_traffic", "mnav_map_timed_traffic")


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mnav.h")).read()
    names = set(re.findall(r"\b(mnav_[a-z_]+)\s*\(", hdr))
    L = C.CDLL(B.build_lib())
    for s in SYMBOLS:
        assert s in names and s in capi.SYMBOLS and hasattr(L, s), s
    for m in ("fleet_timed_traffic", "timed_traffic_download", "timed_traffic_stats", "layer_timed_traffic", "map_timed_traffic"):
        assert hasattr(capi.MnavContext, m), m
    opts = open(os.path.join(ROOT, "mesh_navigation_amd", "csrc", "mnav_options.h")).read()
    assert "X(timed_traffic_max_mb)" in opts


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
