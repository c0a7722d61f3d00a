"""The child processes of tests/test_switches_cpu.py and tests/test_hip_switches.py: the library reads the environment once per
process, so the environment level of a kernel switch (csrc/switches.hpp) is visible only in a process started under it.  Run as a
program this file prints one JSON line:

    python tests/_switches.py precedence    the conv_wino switch through its three levels, seen in a plan's workspace size (no GPU)
    python tests/_switches.py split         the conv_wino_split switch, seen in the kernel names of one 16 x 16 conv launch"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import mcedm_oracle as orc  # noqa: E402

CFG = orc.UNetConfig(ch=128, ch_mult=(1, 1, 1, 1), attn_resolutions=(16,))


def make_plan(L):
    c = CFG
    return L.Plan(c.in_channels, c.cond_channels, c.out_ch, c.ch, c.ch_mult, c.num_res_blocks, c.attn_resolutions, c.resolution)


def size(plan):
    return plan.workspace_bytes(2, 64, 64)


def precedence(L):
    """Workspace sizes after each step of the table in test_three_levels_of_a_switch (the environment is the caller's)."""
    steps = {}
    pa, pb = make_plan(L), make_plan(L)
    steps["fresh"] = size(pa)
    L.set_conv_wino(1)
    steps["process_on"] = size(pa)
    pa.set_variant("conv_wino", 0)
    steps["plan_off"], steps["sibling"] = size(pa), size(pb)
    pa.set_variant("conv_wino", -1)
    steps["plan_default"] = size(pa)
    L.set_conv_wino(-1)
    steps["process_default"] = size(pa)
    return steps


def split(L):
    """Kernel names of the smallest launch the SPLIT Winograd variant serves, under the environment alone, with the process-wide
    switch on, and with it back at its default."""
    from tests import test_hip_wino_split as WS
    fn = WS.conv_launch(L, "wino_split/disp/16x16", 1, 32, 32, 16, 16)
    names = {}
    names["env"] = WS.profiled(L, fn)[1]
    L.set_conv_wino_split(1)
    names["process_on"] = WS.profiled(L, fn)[1]
    L.set_conv_wino_split(-1)
    names["process_default"] = WS.profiled(L, fn)[1]
    return names


if __name__ == "__main__":
    import mcedm_amd  # noqa: F401
    from mcedm_amd import lib
    lib.load()
    print(json.dumps({"precedence": precedence, "split": split}[sys.argv[1]](lib)))
