"""CPU: the fleet rollout's C ABI as built -- the two symbols in the cross-compiled library, in the header and in
capi.SYMBOLS, the ctypes layout of mnav_separation_config against a compiled probe of include/mnav.h, the two flag values,
the two options, and the three k_fleet_rollout_* kernels and the passes of the check in the gfx950 code object inside
libmnav.so (by their names in its symbol table)."""
import ctypes as C
import os
import re
import shutil
import subprocess

from mesh_navigation_amd import build as B
from mesh_navigation_amd import capi
from tests.test_follow_capi_cpu import llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_fleet_rollout_stay", "k_fleet_rollout_search", "k_fleet_rollout_global", "k_sep_clear", "k_sep_insert", "k_sep_sums", "k_sep_top", "k_sep_starts",
           "k_sep_fill", "k_sep_pair")


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mnav.h")).read()
    names = set(re.findall(r"\b(mnav_[a-z_]+)\s*\(", hdr))
    L = C.CDLL(B.build_lib())
    for s in ("mnav_fleet_rollout", "mnav_fleet_rollout_stats"):
        assert s in names and s in capi.SYMBOLS and hasattr(L, s), s
    assert "#define MNAV_SEP_WAITING_PRESENT 1u" in hdr and "#define MNAV_SEP_REACHED_PRESENT 2u" in hdr
    assert (capi.SEP_WAITING_PRESENT, capi.SEP_REACHED_PRESENT) == (1, 2)
    options = open(os.path.join(ROOT, "mesh_navigation_amd", "csrc", "mnav_options.h")).read()
    assert "X(separation_cell_scale)" in options and "X(separation_max_tests)" in options
    # the rollout's own kernels and entry points are still there
    assert "mnav_follow_rollout" in names and hasattr(L, "mnav_follow_rollout") and hasattr(L, "mnav_rollout_stats")


def test_config_layout_and_flag_values_match_the_header(tmp_path):
    fields = [n for n, _ in capi.SeparationConfig._fields_]
    probe = '#include <stddef.h>\n#include <stdio.h>\n#include "mnav.h"\nint main(void) { mnav_separation_config d; printf("%zu", sizeof(mnav_separation_config)); ' + \
            " ".join('printf(" %%zu %%zu", offsetof(mnav_separation_config, %s), sizeof(d.%s));' % (f, f) for f in fields) + \
            ' printf(" %u %u", MNAV_SEP_WAITING_PRESENT, MNAV_SEP_REACHED_PRESENT); return 0; }\n'
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(probe)
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("g++")
    assert cc, "a C compiler is needed for the layout probe"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == C.sizeof(capi.SeparationConfig) == 16
    for k, f in enumerate(fields):
        assert out[1 + 2 * k] == getattr(capi.SeparationConfig, f).offset and out[2 + 2 * k] == getattr(capi.SeparationConfig, f).size, f
    assert fields == ["radius", "check_stride", "flags"]
    assert out[1 + 2 * len(fields):] == [capi.SEP_WAITING_PRESENT, capi.SEP_REACHED_PRESENT]
    sep = capi.SeparationConfig(radius=0.25, check_stride=7)
    assert (sep.radius, sep.check_stride, sep.flags) == (0.25, 7, 0)


def test_the_kernels_are_in_the_gfx950_code_object(tmp_path):
    lib = B.build_lib()
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.check_call([llvm_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "stripped.so")])
    subprocess.check_call([llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    symbols = subprocess.check_output([llvm_tool("llvm-objdump"), "--syms", co], text=True).split()      # the symbol table only
    for k in KERNELS + ("k_rollout_stay", "k_rollout_search", "k_rollout_global"):
        hit = [s for s in symbols if re.fullmatch(r"_Z\w*" + k + r"\w*", s)]                              # (no ".kd", no ".num_vgpr" ...)
        assert len(hit) == 1 and (hit[0] + ".kd") in symbols, (k, hit)       # the function and its kernel descriptor
