"""CPU: the yielding fleet rollout's C ABI as built -- the two symbols in the cross-compiled library, in the header and in
capi.SYMBOLS, the ctypes layout of mnav_yield_config against a compiled probe of include/mnav.h, and the three
k_yield_rollout_* kernels and the pair pass k_yld_pair in the gfx950 code object inside libmnav.so (by their names in its
symbol table), beside the fleet rollout's kernels, which a call without a yield config still runs."""
import ctypes as C
import os
import re
import shutil
import subprocess

from mesh_navigation_amd import build as B
from mesh_navigation_amd import capi
from tests.test_fleet_rollout_capi_cpu import KERNELS as FLEET_KERNELS
from tests.test_follow_capi_cpu import llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_yield_rollout_stay", "k_yield_rollout_search", "k_yield_rollout_global", "k_yld_pair")


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mnav.h")).read()
    names = set(re.findall(r"\b(mnav_[a-z_]+)\s*\(", hdr))
    L = C.CDLL(B.build_lib())
    for s in ("mnav_fleet_rollout_yield", "mnav_fleet_yield_stats"):
        assert s in names and s in capi.SYMBOLS and hasattr(L, s), s
    assert "typedef struct mnav_yield_config" in hdr
    # the wrapper and the entry points it stands beside
    assert hasattr(capi.MnavContext, "fleet_rollout_yield") and hasattr(capi.MnavContext, "fleet_yield_stats")
    assert "mnav_fleet_rollout" in names and hasattr(L, "mnav_fleet_rollout") and hasattr(L, "mnav_fleet_rollout_stats")
    # the yield group follows every argument of mnav_fleet_rollout, in its order
    def args(name):
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr).group(1)
        return [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]
    fleet, yld = args("mnav_fleet_rollout"), args("mnav_fleet_rollout_yield")
    assert yld[: len(fleet)] == fleet
    assert yld[len(fleet):] == ["yield", "priority", "hold_in", "hold_out", "hold_checks_out", "held_ticks_out", "first_hold_tick_out", "first_hold_robot_out"]


def test_config_layout_matches_the_header(tmp_path):
    fields = [n for n, _ in capi.YieldConfig._fields_]
    probe = '#include <stddef.h>\n#include <stdio.h>\n#include "mnav.h"\nint main(void) { mnav_yield_config d; printf("%zu", sizeof(mnav_yield_config)); ' + \
            " ".join('printf(" %%zu %%zu", offsetof(mnav_yield_config, %s), sizeof(d.%s));' % (f, f) for f in fields) + " return 0; }\n"
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(probe)
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("g++")
    assert cc, "a C compiler is needed for the layout probe"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == C.sizeof(capi.YieldConfig) == 16
    for k, f in enumerate(fields):
        assert out[1 + 2 * k] == getattr(capi.YieldConfig, f).offset and out[2 + 2 * k] == getattr(capi.YieldConfig, f).size, f
    assert fields == ["ahead_cos", "flags"]
    y = capi.YieldConfig(ahead_cos=0.25)
    assert (y.ahead_cos, y.flags) == (0.25, 0)


def test_the_kernels_are_in_the_gfx950_code_object(tmp_path):
    lib = B.build_lib()
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.check_call([llvm_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "stripped.so")])
    subprocess.check_call([llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    symbols = subprocess.check_output([llvm_tool("llvm-objdump"), "--syms", co], text=True).split()      # the symbol table only
    for k in KERNELS + FLEET_KERNELS + ("k_rollout_stay", "k_rollout_search", "k_rollout_global"):
        hit = [s for s in symbols if re.fullmatch(r"_Z\w*" + k + r"\w*", s)]                              # (no ".kd", no ".num_vgpr" ...)
        assert len(hit) == 1 and (hit[0] + ".kd") in symbols, (k, hit)       # the function and its kernel descriptor
