"""CPU: what hipcc makes of the GEMM main loop (llama-x_amd/csrc/gemm_bf16.hip), read from the gfx950 assembly.

DESIGN §4 claims a steady-state K loop with no vector address arithmetic and no guards; the compiler has broken that claim before
without anything failing (a 64-bit vector add in front of every LDS-DMA piece, fifteen wave-uniform branches per K-tile), so the claim
is checked where it lives.  The counts are conditions that follow from the tile geometry, not measurements:
  * 256 x 256 tile: a wave owns 128 x 64 outputs = 8 x 4 accumulator tiles x 2 k-steps = 64 MFMAs per K-tile (256 x 128: 4 x 4 x 2 = 32)
  * a K-tile is 4 A pieces + 4 B pieces of 64 rows, one LDS-DMA instruction per thread and piece = 8 (half tile: 4 + 2 = 6)
  * one backward branch closes the loop (one more is allowed for a loop the compiler rotates)
No GPU is needed: the file is cross-compiled with the Makefile's flags.  Skipped where hipcc is absent."""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "llama-x_amd", "csrc")

# (EPI, I8, BNT) -> MFMAs, LDS-DMA instructions per steady K-tile
INSTANCES = {(0, False, 256): (64, 8), (7, False, 256): (64, 8), (6, False, 128): (32, 6), (0, True, 256): (64, 8),
             (5, True, 256): (64, 8)}  # <5, true> is the int8 instance the library launches for "no epilogue"
# <0, true, 1, 256> is not among the library's instances (llx_int8_mm_dequant* map epilogue 0 to EPI_ROWCOLSCALE = 5): it is
# instantiated for this check only, from the same template
EXTRA_INSTANCES = "template __global__ void gemm_nt_kernel<EPI_NONE, true, 1, 256>(const GemmArgs);\n"


def _makefile_vars():
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*\??=\s*(.*)$", text, re.M)}
    hipcc = os.environ.get("HIPCC", var["HIPCC"])
    flags = var["CXXFLAGS"].replace("$(ARCH)", var["ARCH"]).split()
    return hipcc, flags


def _mangled(epi, i8, bnt):
    return f"_Z14gemm_nt_kernelILi{epi}ELb{int(i8)}ELi1ELi{bnt}EEv8GemmArgs"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """name -> assembly text of every gemm_nt_kernel instance (function body + its .amdhsa_kernel descriptor)."""
    hipcc, flags = _makefile_vars()
    if not (os.path.isfile(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("gemm_isa")
    src = tmp / "gemm_isa.hip"
    src.write_text(f'#include "{os.path.join(CSRC, "gemm_bf16.hip")}"\n' + EXTRA_INSTANCES)
    out = tmp / "gemm_isa.s"
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", str(src), "-o", str(out)], check=True, cwd=str(tmp))
    text = out.read_text()
    found = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z14gemm_nt_kernel\w+):[^\n]*\n(.*?^\s*\.end_amdhsa_kernel)", text, re.S | re.M)}
    assert len(found) >= 20, sorted(found)
    return found


def _instructions(lines):
    return [l.split()[0] for l in lines if l.startswith("\t") and not l.lstrip().startswith((".", ";"))]


def _steady_loop(body):
    """Instructions of the first innermost loop that holds MFMAs: the steady-state K loop comes before the guarded tail in the source
    and in the code.  A loop = a label and the last branch back to it, with no other backward branch target in between."""
    lines = body.split("\n")
    label_at = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"(\.LBB\d+_\d+):", l))}
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and label_at.get(m.group(1), len(lines)) <= i:
            loops.append((label_at[m.group(1)], i))
    for a, b in sorted(loops):
        if any((c, d) != (a, b) and a <= c and d <= b for c, d in loops):
            continue  # not innermost
        ins = _instructions(lines[a:b + 1])
        if any(x.startswith("v_mfma") for x in ins):
            return ins
    raise AssertionError("no loop with MFMAs")


@pytest.mark.parametrize("inst", sorted(INSTANCES), ids=lambda t: f"epi{t[0]}-{'i8' if t[1] else 'bf16'}-bnt{t[2]}")
def test_steady_loop_is_bare(kernels, inst):
    n_mfma, n_dma = INSTANCES[inst]
    ins = _steady_loop(kernels[_mangled(*inst)])
    hist = collections.Counter(ins)
    print(inst, len(ins), "instructions:", dict(hist))
    mfma = "v_mfma_i32_16x16x64_i8" if inst[1] else "v_mfma_f32_16x16x32_bf16"
    assert sum(v for k, v in hist.items() if k.startswith("v_mfma")) == n_mfma and hist[mfma] == n_mfma, hist
    dma = [k for k in hist if k.startswith(("buffer_load", "global_load"))]
    assert sum(hist[k] for k in dma) == n_dma and all(k.endswith("dwordx4") for k in dma), hist
    # no 64-bit vector add in any spelling: v_lshl_add_u64 / v_add_u64 / v_add_co(_ci)_u32 carry pairs / v_addc
    wide = [k for k in hist if re.match(r"v_(lshl_add_u64|add_u64|add_co|addc|add_nc_u64|mad_u64|mad_i64)", k)]
    assert not wide, hist
    assert sum(v for k, v in hist.items() if k.startswith(("s_cbranch", "s_branch"))) <= 2, hist
    assert hist["s_barrier"] == 3, hist


def test_steady_loop_dma_form(kernels):
    """Every buffer-form LDS-DMA piece is `buffer_load_dwordx4 v, s[rsrc], s_off offen lds`: descriptor and K position scalar,
    one 32-bit lane offset, and no immediate offset (a large one is dropped without a diagnostic)."""
    for inst in sorted(INSTANCES):
        body = kernels[_mangled(*inst)]
        lines = [l for l in body.split("\n") if re.match(r"\s+buffer_load_dwordx4\b", l)]
        assert lines
        for l in lines:
            assert re.match(r"\s+buffer_load_dwordx4 v\d+, s\[\d+:\d+\], (s\d+|0) offen lds\s*$", l), l


def test_no_scratch_in_any_instance(kernels):
    for name, body in kernels.items():
        m = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        assert m and int(m.group(1)) == 0, (name, m and m.group(1))
