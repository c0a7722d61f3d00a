"""Instruction classes of the Winograd kernels' EPILOGUE -- everything behind the last stage barrier of the loop: the epilogue with
all arms of its branches, init_acc() and the kernel's closing instructions -- counted in the gfx950 assembly by
tools/wino_isa_count.py --epilogue (one device-only compile of csrc/conv_wino.hip, shared by every case; no GPU).

PARENT: the tool run on the parent commit's file.  There the residual loop tested the mode in each of its sixteen iterations (89
branches behind the last stage barrier), the half-resolution arm had a copy and a full wait behind every load (16 of the 22
s_waitcnt vmcnt(0) that sit between two residual loads; 4 more are the double-resolution arm's groups), every 32-lane sum ended in
a ds_bpermute_b32 (16 of the 82 LDS instructions) and the SKIP variant reloaded spilled slot addresses inside the statistics (12
scratch accesses).

What is held, per instantiation (NEW: this commit's counts as upper bounds):
  * s_waitcnt vmcnt(0) between two residual loads: the double-resolution arm keeps its four groups of four channels, each waited
    for before the next is requested -- those four, and in the un-resampled kernels one more in front of the statistics' stores;
    the half-resolution arm is 32 buffer_load_dword and the same-resolution arm 16 buffer_load_dwordx2 with NO instruction that
    waits between the first and the last of them (the first wait is where v0 is formed, behind the exchange's barrier).
  * no scratch access behind the last stage barrier in any kernel but the SKIP variant (parent: one in WinoCfg<2>), two there
    (parent 12).
  * LDS instructions, waits and branches below the parent's; vector-memory: the parent's 84 + the half-resolution arm's second
    sixteen loads (it was 16 loads and 16 copies).
  * spilled registers and scratch bytes of EVERY instantiation not above the parent's.
The vector-instruction count is printed, not bounded: it holds both arms of the hoisted record-width test (pairs / quads), of
which a launch runs one."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = "conv_wino_kernel<"
COLS = ("lds", "vmem", "scratch", "wait", "branch", "vm0_between_loads")
# behind the last stage barrier on the parent commit, columns as COLS
PARENT = {
    K + "WinoCfg<4>, false, true>": (82, 84, 0, 86, 89, 22),
    K + "WinoCfg<4>, false, false>": (82, 84, 0, 86, 89, 22),
    K + "WinoCfg<4>, false, true, WinoBiasRows>": (82, 84, 0, 86, 89, 22),
    K + "WinoCfg<4>, true, true, WinoUp<true> >": (82, 84, 0, 86, 87, 22),
    K + "WinoCfg<2>, false, true>": (82, 84, 1, 87, 89, 23),
    K + "WinoCfg<2>, true, true, WinoUp<true> >": (82, 84, 0, 86, 87, 22),
    K + "WinoSkipCfg<4>, false, true>": (100, 29, 12, 64, 36, 0),
    K + "WinoSplitCfg, false, true>": (53, 20, 0, 54, 26, 1),
    K + "WinoSplitCfg, false, false>": (53, 20, 0, 54, 26, 1),
}
# this commit's
NEW = {
    K + "WinoCfg<4>, false, true>": (66, 100, 0, 58, 28, 5),
    K + "WinoCfg<4>, false, false>": (66, 100, 0, 58, 28, 5),
    K + "WinoCfg<4>, false, true, WinoBiasRows>": (66, 100, 0, 58, 28, 5),
    K + "WinoCfg<4>, true, true, WinoUp<true> >": (66, 100, 0, 55, 26, 4),
    K + "WinoCfg<2>, false, true>": (66, 100, 0, 58, 28, 5),
    K + "WinoCfg<2>, true, true, WinoUp<true> >": (66, 100, 0, 55, 26, 4),
    K + "WinoSkipCfg<4>, false, true>": (84, 29, 2, 41, 34, 0),
    K + "WinoSplitCfg, false, true>": (49, 20, 0, 50, 26, 1),
    K + "WinoSplitCfg, false, false>": (49, 20, 0, 50, 26, 1),
}
# (spilled VGPRs, scratch bytes) of every instantiation on the parent commit
PARENT_SPILLS = {
    "WinoSkipCfg<4>, false, true>": (13, 56), "WinoSkipCfg<4>, false, true, WinoLoop1>": (17, 72),
    "WinoCfg<4>, false, true>": (0, 0), "WinoCfg<4>, false, true, WinoLoop1>": (3, 16),
    "WinoCfg<4>, true, true, WinoLoop1>": (4, 20), "WinoCfg<4>, true, true, WinoUp<true> >": (0, 0),
    "WinoCfg<4>, true, true, WinoLoop1, WinoUp<true> >": (0, 0), "WinoCfg<4>, true, true, WinoUp<false> >": (0, 0),
    "WinoCfg<4>, true, true, WinoLoop1, WinoUp<false> >": (0, 0), "WinoCfg<4>, false, false>": (0, 0),
    "WinoCfg<4>, false, false, WinoLoop1>": (3, 16), "WinoCfg<4>, false, true, WinoBiasRows>": (0, 0),
    "WinoCfg<4>, false, true, WinoLoop1, WinoBiasRows>": (3, 16), "WinoCfg<2>, false, true>": (1, 8),
    "WinoCfg<2>, false, true, WinoLoop1>": (8, 36), "WinoCfg<2>, true, true, WinoLoop1>": (3, 16),
    "WinoCfg<2>, true, true, WinoUp<true> >": (0, 0), "WinoCfg<2>, true, true, WinoLoop1, WinoUp<true> >": (0, 0),
    "WinoCfg<2>, true, true, WinoUp<false> >": (0, 0), "WinoCfg<2>, true, true, WinoLoop1, WinoUp<false> >": (0, 0),
    "WinoCfg<2>, false, false, WinoLoop1>": (8, 36), "WinoCfg<2>, false, true, WinoBiasRows>": (1, 8),
    "WinoCfg<2>, false, true, WinoLoop1, WinoBiasRows>": (8, 36), "WinoSplitCfg, false, true>": (0, 0),
    "WinoSplitCfg, false, true, WinoLoop1>": (0, 0), "WinoSplitCfg, false, false>": (0, 0), "WinoSplitCfg, false, false, WinoLoop1>": (0, 0),
}


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("wino_isa_count", os.path.join(ROOT, "tools", "wino_isa_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def asm(tool):
    return tool.compile_asm()


@pytest.fixture(scope="module")
def epi(tool, asm):
    res = tool.epilogues(asm)
    for name in sorted(res):
        print(f"{name} epilogue: " + " ".join(f"{k} {res[name][k]}" for k in tool.EPI_CLASSES))
    return res


@pytest.mark.parametrize("name", list(NEW))
def test_epilogue_counts_per_instantiation(epi, name):
    assert name in epi, sorted(epi)
    c = epi[name]
    print(f"{name}: valu {c['valu']} mfma {c['mfma']} | " + " ".join(f"{k} {c[k]} (parent {p})" for k, p in zip(COLS, PARENT[name])))
    # init_acc's eight; the SKIP variant: + its projection's 2 + 16; the split kernel's one tile ends the workgroup
    assert c["mfma"] == (26 if "Skip" in name else 0 if "Split" in name else 8), c
    for k, bound in zip(COLS, NEW[name]):
        assert c[k] <= bound, (name, k, c[k], bound)
    for k in ("lds", "wait"):
        assert c[k] < PARENT[name][COLS.index(k)], (name, k, c[k])
    assert c["branch"] <= PARENT[name][COLS.index("branch")]


@pytest.mark.parametrize("name", [K + "WinoCfg<4>, false, true>", K + "WinoCfg<2>, false, true>", K + "WinoCfg<4>, true, true, WinoUp<true> >"])
def test_no_wait_between_the_loads_of_a_straight_line_residual_arm(tool, asm, name):
    ins = tool.instructions(asm)[name]
    for op, n in (("buffer_load_dword", 32), ("buffer_load_dwordx2", 16)):
        runs, cur = [], 0
        for o, _ in ins:
            if o == op:
                cur += 1
            elif o.startswith("s_waitcnt") or o.startswith("s_cbranch") or o in ("s_branch", "s_barrier"):
                if cur:
                    runs.append(cur)
                cur = 0
        print(f"{name}: {op} in runs of {runs} without a wait between them")
        assert n in runs, (name, op, runs)


def test_no_scratch_access_in_the_epilogue_of_the_kernels_without_a_projection(epi):
    for name, c in epi.items():
        if "Skip" not in name:
            assert c["scratch"] == 0, (name, c)


def test_no_instantiation_spills_more_than_the_parent(asm):
    seen = {}
    for blk in asm.split("- .agpr_count:")[1:]:
        get = lambda k: re.search(rf"\.{k}:\s*(\S+)", blk).group(1)
        if "conv_wino_kernel" not in get("name"):
            continue
        name = subprocess.run(["c++filt", get("name")], capture_output=True, text=True, check=True).stdout.strip()
        name = re.sub(r"\(.*$", "", name.replace("void ", "").replace("mcedm::", "")).replace(K, "")
        seen[name] = (int(get("vgpr_count")), int(get("vgpr_spill_count")), int(get("private_segment_fixed_size")))
    assert sorted(seen) == sorted(PARENT_SPILLS), sorted(set(seen) ^ set(PARENT_SPILLS))
    for name, (vgpr, spill, scratch) in sorted(seen.items()):
        print(f"{name}: {vgpr} VGPRs, {spill} spilled (parent {PARENT_SPILLS[name][0]}), {scratch} bytes of scratch (parent {PARENT_SPILLS[name][1]})")
    for name, (vgpr, spill, scratch) in seen.items():
        assert vgpr <= 256 and spill <= PARENT_SPILLS[name][0] and scratch <= PARENT_SPILLS[name][1], (name, vgpr, spill, scratch)
