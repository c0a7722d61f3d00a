"""Instruction classes per K-loop stage of the Winograd kernels, counted in the gfx950 assembly by tools/wino_isa_count.py (one
device-only compile of csrc/conv_wino.hip, ~20 s, shared by every case; no GPU).

fp32 vector instructions do not overlap with the fp32 MFMAs of either wave of a SIMD on gfx950 -- integer ones included
(tools/micro/mfma_valu_coexec.hip) -- so every vector instruction in the K loop is matrix time.  The two-stage
trip forms its addresses outside the loop; this test holds the stage to that.  PARENT: the counts of the commit before the two-stage
trip (the tool run on that commit; per stage and wave): there a stage had 27 address instructions (19 LDS buffer toggles, 6 for the
next chunk's 64-bit weight pointer, the 2 v_mov of the coefficient rows).

Bounds, per stage (both halves of a trip are checked):
  * MFMAs: 64 for the sixteen-position kernels.  WinoUp<true> runs 9 of the 16 positions -- 6 in the hf = 0 waves whose code the
    assembly shows: 2 chunks x 6 positions x 4 k-steps = 48, what the parent has too (a stage of that variant never had 64).
  * floating-point and mask instructions: not above the parent's (72 + 6 plain, 70 + 6 SKIP, 14 + 6 WinoUp<true>).
  * address instructions: <= 6 (parent 27).  What is left: the two v_mov of the coefficient rows' ds_read_b96 and two to four
    v_add_u32 that hipcc's load / store optimiser puts in front of the pairs of ds_write_b32 it merges into ds_write2st64_b32 -- that
    instruction's two offsets are 8 bits each, in units of 256 bytes from ONE base, and the far V buffer lies beyond them.
  * no scratch access inside a stage; registers: <= 256 VGPRs everywhere, spills / scratch of the three flagship forms not above
    the parent's (3 / 16, 16 / 68, 0 / 0; this build: 0 / 0, 13 / 56, 0 / 0).

The floating-point column: a stage has 16 transcendentals and 36 packed fp32 operations, and behind an MFMA hipcc rewrites a packed
operation into two scalar instructions after register allocation -- 18 of the 36 on the parent's SKIP stage (70), 20 and 23 on the new
schedule (72 and 75: above the parent).  The input transform's sixteen are therefore written as instructions (pk_sub / pk_fma /
pk_hi_pm_lo in conv_wino.hip), which stay packed: this build has 58 | 58 (plain), 57 | 61 (SKIP), 14 | 14 (WinoUp<true>)."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# per stage and wave on the parent commit: (mfma, fp, mask, addr)
PARENT = {
    "conv_wino_kernel<WinoCfg<4>, false, true>": (64, 72, 6, 27),
    "conv_wino_kernel<WinoSkipCfg<4>, false, true>": (64, 70, 6, 27),
    "conv_wino_kernel<WinoCfg<4>, true, true, WinoUp<true> >": (48, 14, 6, 19),
}
ADDR_MAX = 6
# (spilled VGPRs, scratch bytes) on the parent commit
PARENT_SPILLS = {
    "conv_wino_kernel<WinoCfg<4>, false, true>": (3, 16),
    "conv_wino_kernel<WinoSkipCfg<4>, false, true>": (16, 68),
    "conv_wino_kernel<WinoSplitCfg, false, true>": (0, 0),
    "conv_wino_kernel<WinoSplitCfg, false, false>": (0, 0),
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
def counts(tool, asm):
    res = tool.count(asm)
    for name in sorted(res):
        for i, c in enumerate(res[name]):
            print(f"{name} stage {i}: " + " ".join(f"{k} {c[k]}" for k in tool.CLASSES))
    return res


@pytest.mark.parametrize("name", list(PARENT))
def test_two_stages_per_trip_with_the_parents_mfmas(counts, name):
    assert name in counts, sorted(counts)
    assert len(counts[name]) == 2, f"{name}: {len(counts[name])} stages found, a trip is two"
    for c in counts[name]:
        assert c["mfma"] == PARENT[name][0], c


@pytest.mark.parametrize("name", list(PARENT))
def test_address_instructions_per_stage(counts, name):
    for i, c in enumerate(counts[name]):
        print(f"{name} stage {i}: {c['addr']} address instructions (parent {PARENT[name][3]})")
        assert c["addr"] <= ADDR_MAX, (name, i, c)


@pytest.mark.parametrize("name", list(PARENT))
def test_floating_point_and_mask_instructions_not_above_the_parents(counts, name):
    for i, c in enumerate(counts[name]):
        print(f"{name} stage {i}: fp {c['fp']} (parent {PARENT[name][1]}), mask {c['mask']} (parent {PARENT[name][2]})")
    for i, c in enumerate(counts[name]):
        assert c["mask"] <= PARENT[name][2], (name, i, c)
        assert c["fp"] <= PARENT[name][1], (name, i, c)


def test_no_scratch_access_inside_a_stage(counts):
    for name, stages in counts.items():
        for i, c in enumerate(stages):
            assert c["scratch"] == 0, (name, i, c)


def test_the_one_stage_form_has_no_more_address_instructions_than_the_parent(counts):
    """WinoLoop1 (odd stage counts per tile) keeps the run-time buffer parity: its stage may not cost more than it did."""
    for name, (_, _, _, addr) in PARENT.items():
        one = name.replace(", true>", ", true, WinoLoop1>") if "WinoUp" not in name else name.replace("WinoUp<true> >", "WinoLoop1, WinoUp<true> >")
        assert one in counts and len(counts[one]) == 1, (one, sorted(counts))
        assert counts[one][0]["addr"] <= addr, (one, counts[one][0])


def test_registers_spills_and_scratch(asm):
    """The kernels' metadata in the same assembly: VGPRs <= 256 for every instantiation, spills and scratch of the flagship forms."""
    import subprocess
    seen = {}
    for blk in asm.split("- .agpr_count:")[1:]:
        get = lambda k: re.search(rf"\.{k}:\s*(\S+)", blk).group(1)
        if "conv_wino_kernel" not in get("name"):
            continue
        name = subprocess.run(["c++filt", get("name")], capture_output=True, text=True, check=True).stdout.strip()
        name = re.sub(r"\(.*$", "", name.replace("void ", "").replace("mcedm::", ""))
        seen[name] = (int(get("vgpr_count")), int(get("vgpr_spill_count")), int(get("private_segment_fixed_size")))
    assert len(seen) >= 20, sorted(seen)
    for name, (vgpr, spill, scratch) in sorted(seen.items()):
        print(f"{name}: {vgpr} VGPRs, {spill} spilled, {scratch} bytes of scratch")
        assert vgpr <= 256, (name, vgpr)
    for name, (spill, scratch) in PARENT_SPILLS.items():
        assert seen[name][1] <= spill and seen[name][2] <= scratch, (name, seen[name])
