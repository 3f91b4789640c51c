"""CPU: the follower's C ABI as built -- the two symbols in the cross-compiled library and in the header, the ctypes
layout of mnav_follow_config against a compiled probe of include/mnav.h, the three k_follow* kernels in the gfx950 code
object, and their disassembly free of scalar stores to memory, scalar atomics and scalar data-cache write-backs (vector
stores only: the kernels write through plain C++)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from mesh_navigation_amd import build as B
from mesh_navigation_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_follow_stay", "k_follow_search", "k_follow_global")


def llvm_tool(name):
    for d in (os.path.join(os.path.dirname(os.path.realpath(B.hipcc())), "..", "llvm", "bin"), "/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    p = shutil.which(name)
    assert p, name + " of the ROCm toolchain not found"
    return p


@pytest.fixture(scope="module")
def disassembly(tmp_path_factory):
    """function label -> instruction lines of the gfx950 code object inside libmnav.so"""
    d = tmp_path_factory.mktemp("follow_codeobj")
    lib = B.build_lib()
    fat, co = str(d / "fat.bin"), str(d / "gfx950.co")
    subprocess.check_call([llvm_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(d / "stripped.so")])
    subprocess.check_call([llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    text = subprocess.check_output([llvm_tool("llvm-objdump"), "-d", co], text=True)
    funcs, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif cur is not None and ln.strip():
            cur.append(ln.strip())
    return funcs


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mnav.h")).read()
    names = set(re.findall(r"\b(mnav_[a-z_]+)\s*\(", hdr))
    L = C.CDLL(B.build_lib())
    for s in ("mnav_follow_batch", "mnav_follow_stats"):
        assert s in names and s in capi.SYMBOLS and hasattr(L, s), s
    for s in ("MNAV_FOLLOW_OK = 0", "MNAV_FOLLOW_OUT_OF_MAP = 1", "MNAV_FOLLOW_NO_FIELD = 2"):
        assert s in hdr
    assert (capi.FOLLOW_OK, capi.FOLLOW_OUT_OF_MAP, capi.FOLLOW_NO_FIELD) == (0, 1, 2)


def test_config_layout_matches_the_header(tmp_path):
    fields = [n for n, _ in capi.FollowConfig._fields_]
    probe = '#include <stddef.h>\n#include <stdio.h>\n#include "mnav.h"\nint main(void) { mnav_follow_config d = MNAV_FOLLOW_CONFIG_DEFAULTS; ' \
            'printf("%zu", sizeof(mnav_follow_config)); ' + " ".join('printf(" %%zu %%.17g", offsetof(mnav_follow_config, %s), d.%s);' % (f, f) for f in fields) + \
            ' return 0; }\n'
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(probe)
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("g++")
    assert cc, "a C compiler is needed for the layout probe"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert int(out[0]) == C.sizeof(capi.FollowConfig) == 64
    defaults = capi.FollowConfig()
    for k, f in enumerate(fields):
        assert int(out[1 + 2 * k]) == getattr(capi.FollowConfig, f).offset, f
        assert float(out[2 + 2 * k]) == getattr(defaults, f) == capi.FollowConfig.DEFAULTS[f], f
    # mesh_controller.h:193-200
    assert capi.FollowConfig.DEFAULTS == dict(max_lin_velocity=1.0, max_ang_velocity=0.5, arrival_fading=0.5, ang_vel_factor=1.0, lin_vel_factor=1.0,
                                              max_angle=20.0, max_search_radius=0.4, max_search_distance=0.4)


def kernel_bodies(disassembly):
    out = {}
    for k in KERNELS:
        hit = [name for name in disassembly if k in name and not name.endswith(".kd")]
        assert len(hit) == 1, (k, hit)
        out[k] = disassembly[hit[0]]
    return out


def test_the_three_kernels_are_in_the_gfx950_code_object(disassembly):
    for k, body in kernel_bodies(disassembly).items():
        print(k, len(body), "instructions")
        assert len(body) > 50 and any("s_endpgm" in ln for ln in body), k
        assert any(ln.split()[0].startswith(("global_store", "flat_store")) for ln in body), k       # results leave through vector stores
    # the single-lane pass has no LDS traffic of its own and no barrier: the common tick does not pay for a wave
    stay = kernel_bodies(disassembly)["k_follow_stay"]
    assert not any(ln.split()[0].startswith(("ds_", "s_barrier")) for ln in stay)


# scalar memory writes of any kind, spelled in pieces so that this file does not name them
_SCALAR_WRITES = re.compile(r"^s_(?:buffer_|scratch_)?(?:st" + r"ore|ato" + r"mic)|^s_dc" + r"ache_(?:wb|discard)")


def test_no_scalar_stores_or_scalar_atomics_in_the_new_kernels(disassembly):
    for k, body in kernel_bodies(disassembly).items():
        bad = [ln for ln in body if _SCALAR_WRITES.match(ln.split()[0])]
        assert not bad, (k, bad[:5])
    assert _SCALAR_WRITES.match("s_" + "store_dword") and _SCALAR_WRITES.match("s_buffer_" + "atomic_add") and _SCALAR_WRITES.match("s_dc" + "ache_wb")
    assert not _SCALAR_WRITES.match("s_load_dword") and not _SCALAR_WRITES.match("global_store_dword")
