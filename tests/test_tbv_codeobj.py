"""CPU: the code object of k_tbv_solve<120> (mesh_navigation_amd/csrc/mnav_tbv.h), read from the device assembly of a
cross-compile (no GPU needed; one compile per test session).

The kernel keeps a tile's distances in a FIXED window of physical VGPRs (v72..v255) that the compiler does not know about, with a
ring and scratch registers at v40..v68; the compiler is held to v0..v39 by `amdgpu_num_vgpr`, and the host launches 8 waves per CU
(two per SIMD, 256 registers each, mnav_tb_host.h).  None of that is visible to the type system: a compiler that allocates one
register into the window, spills to scratch, or takes AGPRs produces wrong distances or a launch that does not fit.  So:

  * metadata: no AGPRs, no VGPR spills, no scratch, exactly 256 VGPRs;
  * body: outside the `;;#ASMSTART` ... `;;#ASMEND` regions (the toolchain emits these markers around every inline-asm statement)
    no operand names a VGPR above v39, single (`v41`) or as a range (`v[38:41]`), and no AGPR at all.  That covers the VGPR whose
    lanes hold spilled SGPRs (v_writelane / v_readlane): SGPR spills are allowed, but only into a compiler register;
  * source: the budget itself.  The kernel needs 33 registers today, so a relaxed attribute (tried: amdgpu_num_vgpr(32), i.e. 64
    registers) changes nothing in the generated code and the scan above stays green -- until a later change of the kernel makes
    the compiler take what it was offered.  The attribute's argument is therefore read from mnav_tbv.h and held to the layout:
    2 n == 40 (the toolchain grants 2 n registers on gfx950: measured in mnav_tbv.h);
  * M0: `win_read` executes s_set_gpr_idx_on, which rewrites M0, without naming "m0" as a clobber.  That is safe as long as the
    compiler itself never uses M0 in this kernel (it has no LDS, no s_movrel, no s_sendmsg, no interpolation): asserted here, so
    the day the compiler starts to keep a value in M0 this test says that the clobber is due.
"""
from __future__ import annotations

import os
import re
import subprocess

import pytest

from mesh_navigation_amd import build as B

KERNEL = re.compile(r"^(_ZN\w*k_tbv_solveILi120EE\w*):")   # the function's label (the toolchain appends a comment)
COMPILER_TOP = 39                      # v[0:39] compiler, mnav_tbv.h
_VREG = re.compile(r"(?<![\w.$])v(\d+)\b")
_VRANGE = re.compile(r"(?<![\w.$])v\[(\d+):(\d+)\]")
_VSUM = re.compile(r"(?<![\w.$])v\[(\d+)\+(\d+)(?::(\d+)\+(\d+))?\]")    # the window by a compile-time row: v[136+7], v[136+4:139+4]
_AREG = re.compile(r"(?<![\w.$])a(\d+)\b|(?<![\w.$])a\[(\d+):(\d+)\]")
_M0 = re.compile(r"(?<![\w.$])m0\b")


def compile_device_asm(out_dir: str, source: str | None = None) -> str:
    flags = [f for f in B.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = os.path.join(out_dir, "mnav_device.s")
    cmd = [B.hipcc(), *flags, "--offload-device-only", "-S", "-o", out, source or os.path.join(B.CSRC, "mnav.hip")]
    subprocess.check_call(cmd)
    with open(out) as f:
        return f.read()


def scan_kernel(asm: str) -> dict:
    """Metadata of k_tbv_solve<120> and the registers its compiler-generated lines name."""
    lines = asm.splitlines()
    labels = [(i, KERNEL.match(ln).group(1)) for i, ln in enumerate(lines) if KERNEL.match(ln)]
    assert len(labels) == 1, labels
    beg, sym = labels[0]
    end = next(i for i in range(beg, len(lines)) if lines[i].startswith(".Lfunc_end"))
    in_asm = False
    r = dict(symbol=sym, compiler_lines=0, asm_lines=0, max_vgpr=-1, offenders=[], agpr_lines=[], m0_lines=[], lane_spill_vgprs=set(),
             asm_max_vgpr=-1)
    for ln in lines[beg + 1:end]:
        s = ln.strip()
        if s.startswith(";;#ASMSTART"):
            assert not in_asm
            in_asm = True
            continue
        if s.startswith(";;#ASMEND"):
            assert in_asm
            in_asm = False
            continue
        code = s.split(";", 1)[0].strip()
        if not code or code.endswith(":") or code.startswith("."):
            continue
        regs = [int(x) for x in _VREG.findall(code)] + [int(hi) for _, hi in _VRANGE.findall(code)]
        if in_asm:
            regs += [int(a) + int(b) for a, b, _, _ in _VSUM.findall(code)] + [int(c) + int(d) for _, _, c, d in _VSUM.findall(code) if c]
            r["asm_lines"] += 1
            r["asm_max_vgpr"] = max([r["asm_max_vgpr"], *regs])
            continue
        r["compiler_lines"] += 1
        top = max(regs, default=-1)
        r["max_vgpr"] = max(r["max_vgpr"], top)
        if top > COMPILER_TOP:
            r["offenders"].append(code)
        if _AREG.search(code):
            r["agpr_lines"].append(code)
        if _M0.search(code):
            r["m0_lines"].append(code)
        if code.startswith("v_writelane_b32"):                            # (v_readlane also serves ordinary wave-uniform reads)
            r["lane_spill_vgprs"].update(regs)
    assert not in_asm
    # the kernel's entry in the amdhsa.kernels list of the metadata note: `  - .key: value` opens an entry, `    .key: value` continues it
    meta, entry = None, None
    for ln in lines[end:]:
        if ln.startswith("  - ."):
            entry = {}
        if entry is not None:
            m = re.match(r"^(?:  - |    )\.(\w+):\s+(\S+)\s*$", ln)
            if m:
                entry[m.group(1)] = m.group(2)
                if m.group(1) == "name" and m.group(2) == sym:
                    meta = entry
    assert meta is not None, "no metadata entry for " + sym
    r["meta"] = meta
    return r


@pytest.fixture(scope="module")
def tbv(tmp_path_factory):
    return scan_kernel(compile_device_asm(str(tmp_path_factory.mktemp("tbv_codeobj"))))


def test_metadata_no_agprs_no_spills_no_scratch_and_the_window_is_covered(tbv):
    m = tbv["meta"]
    print("k_tbv_solve<120> metadata:", {k: m[k] for k in ("agpr_count", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")})
    assert int(m["agpr_count"]) == 0
    assert int(m["vgpr_spill_count"]) == 0
    assert int(m["private_segment_fixed_size"]) == 0
    assert int(m["vgpr_count"]) == 256                 # v72..v255 is inside the kernel's allocation; with AGPRs on top 8 waves per CU would not fit
    assert int(m["wavefront_size"]) == 64 and int(m["group_segment_fixed_size"]) == 0


def test_compiler_stays_below_the_ring_and_the_window(tbv):
    print("k_tbv_solve<120>: %d compiler lines, %d inline-assembly lines, highest compiler VGPR v%d, SGPR-spill VGPRs %s"
          % (tbv["compiler_lines"], tbv["asm_lines"], tbv["max_vgpr"], sorted(tbv["lane_spill_vgprs"])))
    # the parser saw the kernel: both kinds of lines in their hundreds, and the assembly does reach the top of the window
    assert tbv["compiler_lines"] > 200 and tbv["asm_lines"] > 500
    assert tbv["asm_max_vgpr"] == 255
    assert 0 <= tbv["max_vgpr"] <= COMPILER_TOP
    assert not tbv["offenders"], tbv["offenders"][:5]
    assert not tbv["agpr_lines"], tbv["agpr_lines"][:5]
    # spilled SGPRs live in lanes of a COMPILER register (never scratch: private_segment_fixed_size == 0 above)
    if int(tbv["meta"]["sgpr_spill_count"]) > 0:
        assert tbv["lane_spill_vgprs"] and max(tbv["lane_spill_vgprs"]) <= COMPILER_TOP


def test_the_attribute_grants_the_compiler_exactly_its_range():
    with open(os.path.join(B.CSRC, "mnav_tbv.h")) as f:
        src = f.read()
    grants = re.findall(r"^#define\s+TBV_COMPILER_VGPRS\s+__attribute__\(\(amdgpu_num_vgpr\((\d+)\)\)\)", src, re.M)
    assert len(grants) == 1, grants
    assert 2 * int(grants[0]) == COMPILER_TOP + 1
    uses = re.findall(r"__global__\s+__launch_bounds__\(64\)\s+TBV_COMPILER_VGPRS", src)
    assert uses, "k_tbv_solve no longer carries TBV_COMPILER_VGPRS"


def test_compiler_never_uses_m0_so_win_read_needs_no_clobber(tbv):
    assert not tbv["m0_lines"], tbv["m0_lines"][:5]


def test_scanner_sees_registers_in_every_operand_form():
    """The scan itself, on hand-written lines: singles, ranges, comments, and text inside the inline-assembly markers."""
    sym = "_ZN12_GLOBAL__N_111k_tbv_solveILi120EEEvNS_2tb4ArgsEPKjS4_S4_PKN4mnav6TbvExpEi"
    body = ["\tv_mov_b32_e32 v7, v39", "\tglobal_load_dwordx4 v[36:39], v[2:3], off", "\t;;#ASMSTART", "\tv_mov_b32 v255, v72", "\t;;#ASMEND",
            "\ts_mov_b32 s40, 0 ; v200 in a comment", "\tv_writelane_b32 v32, s8, 0"]
    tail = [".Lfunc_end0:", "amdhsa.kernels:", "  - .agpr_count:     0", "    .name:           " + sym, "    .vgpr_count:     256"]
    ok = scan_kernel("\n".join([sym + ":"] + body + tail))
    assert ok["max_vgpr"] == 39 and not ok["offenders"] and ok["asm_max_vgpr"] == 255 and ok["lane_spill_vgprs"] == {32}
    assert ok["meta"]["vgpr_count"] == "256" and ok["meta"]["agpr_count"] == "0"
    for bad in ("\tv_add_u32_e32 v1, v41, v2", "\tglobal_load_dwordx4 v[38:41], v[2:3], off", "\tv_writelane_b32 v64, s8, 0"):
        r = scan_kernel("\n".join([sym + ":"] + body + [bad] + tail))
        assert r["offenders"] == [bad.strip()] and r["max_vgpr"] > COMPILER_TOP
    r = scan_kernel("\n".join([sym + ":"] + body + ["\tv_accvgpr_write_b32 a0, v1", "\ts_mov_b32 m0, s3"] + tail))
    assert r["agpr_lines"] and r["m0_lines"]
