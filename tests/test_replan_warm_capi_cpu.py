"""CPU: the warm repair's C ABI as built -- mnav_replan_warm_stats in the cross-compiled library, in the header and in
capi.SYMBOLS, its Python binding, the two options, the refusal of a call without a context, and k_tb_warm (mnav_tb_warm.h)
in the gfx950 code object inside libmnav.so (by its name in the symbol table)."""
import ctypes as C
import os
import re
import subprocess

from mesh_navigation_amd import build as B
from mesh_navigation_amd import capi
from tests.test_follow_capi_cpu import llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_tb_warm",)


def test_the_symbol_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mnav.h")).read()
    names = set(re.findall(r"\b(mnav_[a-z_]+)\s*\(", hdr))
    L = C.CDLL(B.build_lib())
    s = "mnav_replan_warm_stats"
    assert s in names and s in capi.SYMBOLS and hasattr(L, s), s
    assert hasattr(capi.MnavContext, "replan_warm_stats")
    opts = open(os.path.join(ROOT, "mesh_navigation_amd", "csrc", "mnav_options.h")).read()
    assert "X(replan_repair_engine)" in opts and "X(replan_warm_min_plans)" in opts


def test_a_call_without_a_context_is_refused():
    L = capi.load()
    assert L.mnav_replan_warm_stats(None, *([None] * 8)) == -1


def test_the_engine_names_of_a_warm_repair():
    """what MnavContext.last_engine() makes of mnav_last_engine's warm bits (512, 1024) needs no device"""
    assert "k_tb_warm" in capi._warm_name(0) and "k_tb_solve_q" in capi._warm_name(0)
    assert "k_tb_warm" in capi._warm_name(1) and "k_tbv_solve" in capi._warm_name(1)


def test_the_kernel_is_in_the_gfx950_code_object(tmp_path):
    lib = B.build_lib()
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.check_call([llvm_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "stripped.so")])
    subprocess.check_call([llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    symbols = subprocess.check_output([llvm_tool("llvm-objdump"), "--syms", co], text=True).split()      # the symbol table only
    for k in KERNELS:
        hit = [s for s in symbols if re.fullmatch(r"_Z\w*" + k + r"\w*", s)]                              # (no ".kd", no ".num_vgpr" ...)
        assert len(hit) == 1 and (hit[0] + ".kd") in symbols, (k, hit)       # the function and its kernel descriptor
