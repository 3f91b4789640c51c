"""CPU: the per-plan replan's C ABI as built -- the two symbols in the cross-compiled library, in the header and in
capi.SYMBOLS, their Python bindings, the option, the refusal of a call without a context, and the k_replan_* kernels of
mnav_replan_each.h in the gfx950 code object inside libmnav.so (by their names in its symbol table)."""
import ctypes as C
import os
import re
import subprocess

from mesh_navigation_amd import build as B
from mesh_navigation_amd import capi
from tests.test_follow_capi_cpu import llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_replan_open", "k_replan_classify", "k_replan_gather")


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mnav.h")).read()
    names = set(re.findall(r"\b(mnav_[a-z_]+)\s*\(", hdr))
    L = C.CDLL(B.build_lib())
    for s in ("mnav_replan_dijkstra_each", "mnav_replan_each_stats"):
        assert s in names and s in capi.SYMBOLS and hasattr(L, s), s
    assert hasattr(capi.MnavContext, "replan_dijkstra_each") and hasattr(capi.MnavContext, "replan_each_stats")
    opts = open(os.path.join(ROOT, "mesh_navigation_amd", "csrc", "mnav_options.h")).read()
    assert "X(replan_each_fresh_share)" in opts


def test_a_call_without_a_context_is_refused():
    """(The refusal before any Dijkstra call needs a context, hence a device: tests/test_gpu_replan_each.py.)"""
    L = capi.load()
    assert L.mnav_replan_dijkstra_each(None, 1, None, 0.3, None, None, None, None, 0, None) == capi.INTERNAL_ERROR
    assert L.mnav_replan_each_stats(None, *([None] * 12)) == -1


def test_the_kernels_are_in_the_gfx950_code_object(tmp_path):
    lib = B.build_lib()
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.check_call([llvm_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "stripped.so")])
    subprocess.check_call([llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    symbols = subprocess.check_output([llvm_tool("llvm-objdump"), "--syms", co], text=True).split()      # the symbol table only
    for k in KERNELS:
        hit = [s for s in symbols if re.fullmatch(r"_Z\w*" + k + r"\w*", s)]                              # (no ".kd", no ".num_vgpr" ...)
        assert len(hit) == 1 and (hit[0] + ".kd") in symbols, (k, hit)       # the function and its kernel descriptor
