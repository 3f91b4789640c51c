"""CPU: the sampled rollout's C ABI as built -- the two symbols in the cross-compiled library, in the header and in
capi.SYMBOLS, the ctypes layout of mnav_sample_config against a compiled probe of include/mnav.h, and the five k_sample_*
kernels in the gfx950 code object inside libmnav.so (by their names in its symbol table), beside the rollout's kernels,
which mnav_follow_rollout still runs."""
import ctypes as C
import os
import re
import shutil
import subprocess

from mesh_navigation_amd import build as B
from mesh_navigation_amd import capi
from tests.test_follow_capi_cpu import llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_sample_expand", "k_sample_stay", "k_sample_search", "k_sample_global", "k_sample_score", "k_sample_pick")


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mnav.h")).read()
    names = set(re.findall(r"\b(mnav_[a-z_]+)\s*\(", hdr))
    L = C.CDLL(B.build_lib())
    for s in ("mnav_follow_sample", "mnav_sample_stats"):
        assert s in names and s in capi.SYMBOLS and hasattr(L, s), s
    assert "typedef struct mnav_sample_config" in hdr and "#define MNAV_SAMPLE_CONFIG_DEFAULTS" in hdr
    assert hasattr(capi.MnavContext, "follow_sample") and hasattr(capi.MnavContext, "sample_stats")
    # the robots and the two configs come first, as mnav_follow_rollout takes them; then the table, the sample config, the picks, the rows
    def args(name):
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr).group(1)
        return [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]
    rollout, sample = args("mnav_follow_rollout"), args("mnav_follow_sample")
    assert sample[:12] == rollout[:12] and rollout[11] == "rollout"
    assert sample[12:] == ["n_candidates", "candidates", "sample"] + [k + "_out" for k in capi.SAMPLE_PICKS + capi.SAMPLE_ROWS]
    assert len(args("mnav_sample_stats")) == 14


def test_config_layout_matches_the_header(tmp_path):
    fields = [n for n, _ in capi.SampleConfig._fields_]
    probe = '#include <stddef.h>\n#include <stdio.h>\n#include "mnav.h"\nint main(void) { mnav_sample_config d = MNAV_SAMPLE_CONFIG_DEFAULTS; ' + \
            'printf("%zu", sizeof(mnav_sample_config)); ' + \
            " ".join('printf(" %%zu %%zu", offsetof(mnav_sample_config, %s), sizeof(d.%s));' % (f, f) for f in fields) + \
            ' printf(" %g %g %g %g %u", d.w_potential, d.w_cost, d.w_time, d.lethal_cost, d.flags); return 0; }\n'
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(probe)
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("g++")
    assert cc, "a C compiler is needed for the layout probe"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split()
    sizes, defaults = [int(x) for x in out[: 1 + 2 * len(fields)]], [float(x) for x in out[1 + 2 * len(fields):]]
    assert sizes[0] == C.sizeof(capi.SampleConfig) == 40
    for k, f in enumerate(fields):
        assert sizes[1 + 2 * k] == getattr(capi.SampleConfig, f).offset and sizes[2 + 2 * k] == getattr(capi.SampleConfig, f).size, f
    assert fields == ["w_potential", "w_cost", "w_time", "lethal_cost", "flags"]
    s = capi.SampleConfig()
    assert defaults == [s.w_potential, s.w_cost, s.w_time, s.lethal_cost, s.flags] == [1.0, 0.0, 0.0, 1.0, 0]      # the macro and the wrapper agree
    s = capi.SampleConfig(w_cost=0.25, lethal_cost=float("inf"))
    assert (s.w_potential, s.w_cost, s.lethal_cost, s.flags) == (1.0, 0.25, float("inf"), 0)


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
