#!/usr/bin/env python
"""Instruction classes per K-loop stage, and of the epilogue, of the Winograd conv kernels (device-only compile to assembly, no GPU needed).

    python tools/wino_isa_count.py [--epilogue] [substring-filter ...]

conv_wino.hip is compiled for gfx950 with the flags of m-cedm_amd/build.py plus --cuda-device-only -S into a temporary
directory.  In every conv_wino_kernel instantiation a STAGE is the run of basic blocks in front of an s_barrier that hold
the stage's MFMAs (64 per wave in the sixteen-position kernels: 2 chunks x 8 positions x 4 k-steps, or 32 + 32 with one chunk
per stage; 48 in the zero-position up-sampling kernel's hf = 0 waves; 16 in the split kernel); blocks without an MFMA between
them (the tile geometry of raw_load_next, taken once per tile) are not part of it.  Per stage the tool prints the number of
    mfma   v_mfma_*
    fp     floating-point vector instructions (v_*_f32 / v_*_f16 / v_pk_*_f32, conversions and transcendentals included)
    mask   v_and_b32, v_cndmask_b32
    addr   v_add_u32, v_lshl_add_u32, v_add_lshl_u32, v_lshl_add_u64, v_add_co_u32, v_addc_co_u32, v_mad_u64_u32, v_mov_b32
    lds    ds_*
    vmem   global_* / buffer_* / flat_*
    scratch  scratch_* (spill code inside the stage)
    other  any other vector instruction (v_*)
--epilogue: the EPILOGUE instead -- everything behind the last stage barrier of the loop in program order: the epilogue with all arms of
its branches (hipcc lays some of them out behind the kernel's end), init_acc() and the kernel's few closing instructions:
    valu   vector instructions other than MFMAs        mfma   v_mfma_* (init_acc's; the SKIP variant: its projection's too)
    lds    ds_*          vmem   global_* / buffer_* / flat_*          scratch   scratch_*
    wait   s_waitcnt     branch   s_cbranch_* / s_branch             barrier   s_barrier
    vm0_between_loads    s_waitcnt with vmcnt(0) between the first and the last buffer_load of the epilogue: a wait for every load in
                         flight in front of a further residual load
It counts instruction classes only.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "m-cedm_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}",
         "-Wall", "-Wno-unused-function"]           # = build.py's COMMON
ADDR = {"v_add_u32", "v_lshl_add_u32", "v_add_lshl_u32", "v_lshl_add_u64", "v_add_co_u32", "v_addc_co_u32", "v_mad_u64_u32",
        "v_mov_b32"}
MASK = {"v_and_b32", "v_cndmask_b32"}
CLASSES = ("mfma", "fp", "mask", "addr", "lds", "vmem", "scratch", "other")


def classify(op):
    op = re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("scratch_"):
        return "scratch"
    if op.split("_")[0] in ("global", "buffer", "flat"):
        return "vmem"
    if not op.startswith("v_"):
        return None                                 # scalar instructions, waits, branches
    if op in ADDR:
        return "addr"
    if op in MASK:
        return "mask"
    if re.search(r"_(f32|f16|f64|bf16)$", op) or re.search(r"_(f32|f16)_", op):
        return "fp"
    return "other"


def compile_asm(src=None, extra=()):
    """gfx950 assembly of conv_wino.hip as text"""
    src = src or os.path.join(CSRC, "conv_wino.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "conv_wino.s")
        cmd = [HIPCC] + FLAGS + os.environ.get("MCEDM_EXTRA_HIPCC_FLAGS", "").split() + list(extra) + ["--cuda-device-only", "-S", src, "-o", out]
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()


def functions(asm):
    """{demangled kernel name: [basic blocks]}, a basic block = list of mnemonics; a block ends at a label or behind a branch"""
    funcs, name, blocks = {}, None, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, blocks = m.group(1), [[]]
            funcs[name] = blocks
            continue
        if name is None:
            continue
        if re.match(r"^\.Lfunc_end", line):
            name = None
            continue
        if re.match(r"^\.LBB\w+:", line):
            if blocks[-1]:
                blocks.append([])
            continue
        m = re.match(r"^\s+([a-z]\w+)", line)
        if not m:
            continue
        op = m.group(1)
        blocks[-1].append(op)
        if op.startswith("s_cbranch") or op == "s_branch":
            blocks.append([])
    mangled = [n for n in funcs if "conv_wino_kernel" in n]
    if not mangled:
        return {}
    dem = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for n, d in zip(mangled, dem):
        d = re.sub(r"^void mcedm::", "", d.strip())
        d = re.sub(r"\(.*$", "", d).replace("mcedm::", "")
        out[d] = [b for b in funcs[n] if b]
    return out


def stage_mfmas(name):
    """MFMAs per stage and wave of an instantiation (the docstring)"""
    if "WinoSplitCfg" in name:
        return 16
    one = "Cfg<2>" in name                          # one chunk per stage
    if "WinoUp<" in name:
        return 24 if one else 48
    return 32 if one else 64


def stages(blocks, want):
    """[{class: count}] for every stage of one kernel, in program order"""
    found = []
    for bi, blk in enumerate(blocks):
        for pos, op in enumerate(blk):
            if op != "s_barrier":
                continue
            # walk back from the barrier over the blocks with MFMAs, up to the previous barrier
            picked, total, j = [], 0, bi
            while j >= 0 and total < want:
                part = blk[:pos] if j == bi else blocks[j]
                prev = max((k for k, o in enumerate(part) if o == "s_barrier"), default=-1)
                part = part[prev + 1:]
                n = sum(1 for o in part if classify(o) == "mfma")
                if n:
                    picked.append(part)
                    total += n
                if prev >= 0:
                    break
                j -= 1
            if total != want:
                continue
            c = dict.fromkeys(CLASSES, 0)
            for part in picked:
                for o in part:
                    k = classify(o)
                    if k:
                        c[k] += 1
            c["blocks"] = len(picked)
            found.append(c)
    return found


EPI_CLASSES = ("valu", "mfma", "lds", "vmem", "scratch", "wait", "branch", "barrier", "vm0_between_loads")


def instructions(asm):
    """{demangled kernel name: [(mnemonic, operands)]} in program order"""
    funcs, name = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            funcs[name] = []
            continue
        if name is None:
            continue
        if re.match(r"^\.Lfunc_end", line):
            name = None
            continue
        m = re.match(r"^\s+([a-z]\w+)\s*([^;]*)", line)
        if m:
            funcs[name].append((m.group(1), m.group(2).strip()))
    mangled = [n for n in funcs if "conv_wino_kernel" in n]
    if not mangled:
        return {}
    dem = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for n, d in zip(mangled, dem):
        d = re.sub(r"^void mcedm::", "", d.strip())
        out[re.sub(r"\(.*$", "", d).replace("mcedm::", "")] = funcs[n]
    return out


def epilogue_of(ins, want):
    """{class: count} of one kernel's epilogue, or None if the kernel has no stage"""
    last, prev, n = None, -1, 0
    for i, (op, _) in enumerate(ins):
        if classify(op) == "mfma":
            n += 1
        if op == "s_barrier":
            if n == want:
                last = i
            prev, n = i, 0
    if last is None:
        return None
    region = ins[last + 1:]
    c = dict.fromkeys(EPI_CLASSES, 0)
    loads = [i for i, (op, _) in enumerate(region) if op.startswith("buffer_load")]
    for i, (op, args) in enumerate(region):
        k = classify(op)
        if k == "mfma":
            c["mfma"] += 1
        elif k in ("lds", "vmem", "scratch"):
            c[k] += 1
        elif k is not None:
            c["valu"] += 1
        elif op.startswith("s_waitcnt"):
            c["wait"] += 1
            if loads and loads[0] < i < loads[-1] and "vmcnt(0)" in args:
                c["vm0_between_loads"] += 1
        elif op.startswith("s_cbranch") or op == "s_branch":
            c["branch"] += 1
        elif op == "s_barrier":
            c["barrier"] += 1
    return c


def epilogues(asm=None):
    """{kernel name: epilogue counts} of every conv_wino_kernel instantiation that has a stage"""
    out = {}
    for name, ins in instructions(asm if asm is not None else compile_asm()).items():
        c = epilogue_of(ins, stage_mfmas(name))
        if c:
            out[name] = c
    return out


def count(asm=None):
    """{kernel name: [stage counts]} of every conv_wino_kernel instantiation that has a stage"""
    out = {}
    for name, blocks in functions(asm if asm is not None else compile_asm()).items():
        st = stages(blocks, stage_mfmas(name))
        if st:
            out[name] = st
    return out


def main(argv):
    if "--epilogue" in argv:
        argv = [a for a in argv if a != "--epilogue"]
        src = os.environ.get("MCEDM_WINO_SRC")               # another copy of the file (a parent commit's, for comparison)
        res = epilogues(compile_asm(src) if src else None)
        for name in sorted(res):
            if not argv or any(a in name for a in argv):
                print(f"{name[:76]:76s} epilogue: " + " ".join(f"{k} {res[name][k]}" for k in EPI_CLASSES))
        return 0
    res = count()
    for name in sorted(res):
        if argv and not any(a in name for a in argv):
            continue
        for i, c in enumerate(res[name]):
            print(f"{name[:76]:76s} stage {i}: " + " ".join(f"{k} {c[k]:3d}" for k in CLASSES) + f"  ({c['blocks']} blocks)")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
