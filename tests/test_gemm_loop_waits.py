"""CPU: the hand-counted LDS waits of the GEMM main loop (llama-x_amd/csrc/gemm_bf16.hip), replayed on the gfx950 assembly.

The loop issues its fragment reads as inline asm (`ds_read_b128`) and waits for them with `s_waitcnt lgkmcnt(N)` counted by hand, so
that the MFMAs of a k-step start as soon as THEIR fragments are in.  The compiler neither checks those counts nor keeps the MFMAs on
their side of a wait unless the source pins them there, so the compiled steady loop is replayed here with a model of the counter:
LDS reads return in order, `lgkmcnt(N)` retires all but the youngest N.  Every condition follows from the tile geometry (MH = 16-row
A fragments per phase pair: 4 in the 256-wide tile, 2 in the 128-wide one); none is a measurement:
  * nothing but `ds_read_b128` uses the counter inside the loop (no scalar loads, no other LDS instruction), so the model is exact
  * 8 B fragments + 2 k-steps x 2 halves x MH A fragments = 8 + 4 MH reads per K-tile
  * no MFMA reads a register whose read is still outstanding
  * no read is outstanding at a barrier (a barrier releases a tile for the next LDS-DMA: a read still in flight would race it)
  * at the first MFMA after a group of reads at least one read is still outstanding (the MFMAs do start early)
  * a counted wait is followed by the MH x 2 MFMAs of its k-step before the next wait
  * bf16: exactly MH reads (second A half, k-step 0) sit between the phase-0-end barrier and phase 1's first MFMA; int8: none
  * no AGPR moves and no scratch in the loop
No GPU is needed: the file is cross-compiled with the Makefile's flags.  Skipped where hipcc is absent."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "llama-x_amd", "csrc")

# (EPI, I8, BNT) -> MH
INSTANCES = {(0, False, 256): 4, (7, False, 256): 4, (6, False, 128): 2, (5, True, 256): 4}


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
    tmp = tmp_path_factory.mktemp("gemm_waits")
    out = tmp / "gemm_bf16.s"
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", os.path.join(CSRC, "gemm_bf16.hip"), "-o", str(out)], check=True, cwd=str(tmp))
    text = out.read_text()
    found = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z14gemm_nt_kernel\w+):[^\n]*\n(.*?^\s*\.end_amdhsa_kernel)", text, re.S | re.M)}
    assert len(found) >= 20, sorted(found)
    return found


def _steady_loop(body):
    """Instruction lines (mnemonic + operands, comments stripped) of the first innermost loop that holds MFMAs: the steady-state K loop
    comes before the guarded tail in the source and in the code."""
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
        ins = [l.split(";")[0].strip() for l in lines[a:b + 1] if l.startswith("\t") and not l.lstrip().startswith((".", ";"))]
        ins = [l for l in ins if l]
        if any(l.startswith("v_mfma") for l in ins):
            return ins
    raise AssertionError("no loop with MFMAs")


def _vregs(operand_text):
    """the set of VGPR numbers named in an operand string (v12, v[12:15])"""
    regs = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", operand_text):
        if m.group(3) is not None:
            regs.add(int(m.group(3)))
        else:
            regs.update(range(int(m.group(1)), int(m.group(2)) + 1))
    return regs


def _lgkm_limit(ins):
    """N of an s_waitcnt that bounds lgkmcnt, else None (gfx9 encoding of the plain-number form: bits 11:8)"""
    ops = ins.split(None, 1)[1] if " " in ins else ""
    m = re.search(r"lgkmcnt\((\d+)\)", ops)
    if m:
        return int(m.group(1))
    if re.fullmatch(r"(0x[0-9a-fA-F]+|\d+)", ops.strip()):
        return (int(ops.strip(), 0) >> 8) & 15
    return None


def _replay(loop, mh, early):
    """Walks the loop twice (the second pass starts from the state the first one leaves) and checks every MFMA and barrier."""
    pending = []  # destination register sets of the reads still outstanding, oldest first
    events = []   # per pass: ('read' | 'mfma' | 'barrier')
    ends = []
    for _ in range(2):
        reads_since_mfma = 0
        for ins in loop:
            op = ins.split()[0]
            if op == "ds_read_b128":
                dst = _vregs(ins.split(None, 1)[1].split(",")[0])
                assert len(dst) == 4, ins
                pending.append(dst)
                reads_since_mfma += 1
                events.append("read")
            elif op == "s_waitcnt":
                n = _lgkm_limit(ins)
                if n is not None and len(pending) > n:
                    del pending[:len(pending) - n]
                if n is not None:
                    events.append("wait" if n else "wait0")
            elif op.startswith("v_mfma"):
                src = _vregs(ins.split(None, 1)[1].split(",", 1)[1])
                for dst in pending:
                    assert not (src & dst), f"{ins}: reads v{sorted(src & dst)} while its ds_read_b128 is outstanding ({len(pending)} pending)"
                if reads_since_mfma:
                    assert pending, f"{ins}: first MFMA after {reads_since_mfma} reads waits for all of them"
                reads_since_mfma = 0
                events.append("mfma")
            elif op == "s_barrier":
                assert not pending, f"{len(pending)} ds_read_b128 outstanding at s_barrier"
                events.append("barrier")
        ends.append([sorted(p) for p in pending])
    assert ends[0] == ends[1], ends
    # reads between each barrier and the next MFMA (the loop may be rotated: a barrier of the first pass looks on into the second)
    half = len(events) // 2
    after = []
    for i in range(half):
        if events[i] == "barrier":
            n = 0
            for e in events[i + 1:]:
                if e == "mfma":
                    break
                n += e == "read"
            after.append(n)
    assert sorted(after) == sorted([8 + 2 * mh, mh if early else 0, 0]), after
    # a counted wait (N > 0) releases ONE k-step of a quadrant: MH x 2 MFMAs run before the next wait, no more (a compiler that sinks
    # the k-step's MFMAs below the next wait satisfies everything above and starts nothing early)
    for i in range(half):
        if events[i] == "wait":
            n = 0
            for e in events[i + 1:]:
                if e in ("wait", "wait0"):
                    break
                n += e == "mfma"
            assert n == 2 * mh, (n, events[:half])


@pytest.mark.parametrize("inst", sorted(INSTANCES), ids=lambda t: f"epi{t[0]}-{'i8' if t[1] else 'bf16'}-bnt{t[2]}")
def test_fragment_waits(kernels, inst):
    mh = INSTANCES[inst]
    loop = _steady_loop(kernels[_mangled(*inst)])
    ops = [l.split()[0] for l in loop]
    print(inst, len(loop), "instructions;", [l for l in loop if l.startswith("s_waitcnt")])
    # the LDS reads are the only users of lgkmcnt: the counter model is exact and the reads return in order
    assert not [o for o in ops if o.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime", "s_sendmsg", "s_getreg"))], ops
    assert {o for o in ops if o.startswith("ds_")} == {"ds_read_b128"}, sorted(set(ops))
    assert not [o for o in ops if o.startswith(("flat_", "v_accvgpr", "scratch_"))], ops
    assert ops.count("ds_read_b128") == 8 + 4 * mh, ops.count("ds_read_b128")
    assert ops.count("s_barrier") == 3
    _replay(loop, mh, early=not inst[1])


def test_registers_and_scratch(kernels):
    """every instance fits the 256 architectural VGPRs of two waves per SIMD without scratch"""
    for name, body in kernels.items():
        scratch = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        vgpr = re.search(r"\.amdhsa_next_free_vgpr (\d+)", body)
        assert scratch and int(scratch.group(1)) == 0, (name, scratch and scratch.group(1))
        assert vgpr and int(vgpr.group(1)) <= 256, (name, vgpr and vgpr.group(1))
