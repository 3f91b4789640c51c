"""CPU: the rollout's C ABI as built -- the two symbols in the cross-compiled library, in the header and in capi.SYMBOLS,
the ctypes layout of mnav_rollout_config against a compiled probe of include/mnav.h, the four status values, and the three
k_rollout_* kernels in the gfx950 code object inside libmnav.so (by their names in its symbol table)."""
import ctypes as C
import os
import re
import shutil
import subprocess

from mesh_navigation_amd import build as B
from mesh_navigation_amd import capi
from tests.test_follow_capi_cpu import llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_rollout_stay", "k_rollout_search", "k_rollout_global")


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mnav.h")).read()
    names = set(re.findall(r"\b(mnav_[a-z_]+)\s*\(", hdr))
    L = C.CDLL(B.build_lib())
    for s in ("mnav_follow_rollout", "mnav_rollout_stats"):
        assert s in names and s in capi.SYMBOLS and hasattr(L, s), s
    assert "MNAV_ROLLOUT_RUNNING = 0, MNAV_ROLLOUT_REACHED = 1, MNAV_ROLLOUT_OUT_OF_MAP = 2, MNAV_ROLLOUT_NO_FIELD = 3" in hdr
    assert (capi.ROLLOUT_RUNNING, capi.ROLLOUT_REACHED, capi.ROLLOUT_OUT_OF_MAP, capi.ROLLOUT_NO_FIELD) == (0, 1, 2, 3)


def test_config_layout_and_status_values_match_the_header(tmp_path):
    fields = [n for n, _ in capi.RolloutConfig._fields_]
    enums = ("MNAV_ROLLOUT_RUNNING", "MNAV_ROLLOUT_REACHED", "MNAV_ROLLOUT_OUT_OF_MAP", "MNAV_ROLLOUT_NO_FIELD")
    probe = '#include <stddef.h>\n#include <stdio.h>\n#include "mnav.h"\nint main(void) { mnav_rollout_config d; printf("%zu", sizeof(mnav_rollout_config)); ' + \
            " ".join('printf(" %%zu %%zu", offsetof(mnav_rollout_config, %s), sizeof(d.%s));' % (f, f) for f in fields) + \
            " ".join('printf(" %%d", (int)%s);' % e for e in enums) + ' return 0; }\n'
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(probe)
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("g++")
    assert cc, "a C compiler is needed for the layout probe"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == C.sizeof(capi.RolloutConfig) == 32
    for k, f in enumerate(fields):
        assert out[1 + 2 * k] == getattr(capi.RolloutConfig, f).offset and out[2 + 2 * k] == getattr(capi.RolloutConfig, f).size, f
    assert fields == ["dt", "dist_tolerance", "angle_tolerance", "ticks", "trace_stride"]
    assert out[1 + 2 * len(fields):] == [0, 1, 2, 3]
    ro = capi.RolloutConfig(dt=0.25, ticks=7)
    assert (ro.dt, ro.ticks, ro.trace_stride) == (0.25, 7, 0)


def test_the_three_kernels_are_in_the_gfx950_code_object(tmp_path):
    lib = B.build_lib()
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.check_call([llvm_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "stripped.so")])
    subprocess.check_call([llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    symbols = subprocess.check_output([llvm_tool("llvm-objdump"), "--syms", co], text=True).split()      # the symbol table only
    for k in KERNELS:
        hit = [s for s in symbols if re.fullmatch(r"_Z\w*" + k + r"\w*", s)]                              # (no ".kd", no ".num_vgpr" ...)
        assert len(hit) == 1 and (hit[0] + ".kd") in symbols, (k, hit)       # the function and its kernel descriptor
