"""The kernel-variant switches (csrc/switches.hpp) without a GPU: the table's rows against every other place that names a switch,
and the three levels a switch is resolved at -- the plan's own choice, the process-wide mcedm_op_set_*, the environment -- seen
through conv_wino, the one switch whose effect shows on the host (it changes the workspace layout)."""
import glob
import json
import os
import re
import subprocess
import sys

import pytest

import mcedm_amd  # noqa: F401
from mcedm_amd import lib as L
from tests import _switches as SW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "m-cedm_amd", "csrc")


def table_rows():
    """[(binding name, environment variable, default)] in enumerator order."""
    src = open(os.path.join(CSRC, "switches.hpp")).read()
    return [(n, e, int(d)) for n, e, d in re.findall(r'^\s*\{"([a-z0-9_]+)",\s*"(MCEDM_[A-Z0-9_]+)",\s*(-?\d+)\},', src, flags=re.M)]


def test_every_place_that_names_a_switch_agrees_with_the_table():
    rows = table_rows()
    assert len(rows) == len(L.VARIANTS) == 10, rows
    hdr = open(os.path.join(ROOT, "include", "mcedm_hip.h")).read()
    defines = {n: (int(i), c) for n, i, c in re.findall(r"#define MCEDM_VARIANT_([A-Z0-9_]+) (\d+)\s*/\*(.*?)\*/", hdr, flags=re.S)}
    assert len(defines) == len(rows), sorted(defines)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    doc = doc[doc.index("## Environment switches"):]
    documented = {n: int(d) for n, d in re.findall(r"`(MCEDM_[A-Z0-9_]+)` \((-?\d+)\)", doc)}
    for index, (name, env, default) in enumerate(rows):
        at, comment = defines[name.upper()]
        assert at == index, (name, at, index)
        assert re.search(r"\(env (MCEDM_[A-Z0-9_]+), default (-?\d+)\)", comment).groups() == (env, str(default)), (name, comment)
        assert L.VARIANTS[name] == index, name
        assert "mcedm_op_set_" + name in L.OP_EXPORTS, name
        assert callable(getattr(L, "set_" + name)) and getattr(L, "set_" + name).__doc__, name
        assert documented.get(env) == default, (env, documented.get(env), default)


def test_the_environment_is_read_in_one_file():
    left = {os.path.basename(p): open(p).read().count("getenv(") for p in glob.glob(os.path.join(CSRC, "*.h*"))}
    left = {f: n for f, n in left.items() if n and f != "switches.hip"}
    assert not left, left


def test_three_levels_of_a_switch():
    """First hit wins: the plan's value, the process-wide value, the environment (read once, here MCEDM_WINOGRAD=0 in a child)."""
    plan = SW.make_plan(L)
    on = SW.size(plan)
    plan.set_variant("conv_wino", 0)
    off = SW.size(plan)
    assert on != off
    r = subprocess.run([sys.executable, SW.__file__, "precedence"], env=dict(os.environ, MCEDM_WINOGRAD="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    steps = json.loads(r.stdout.strip().splitlines()[-1])
    assert steps == {"fresh": off, "process_on": on, "plan_off": off, "sibling": on, "plan_default": on, "process_default": off}, (steps, on, off)


def test_a_plan_takes_on_off_or_default_and_the_process_any_integer():
    plan = SW.make_plan(L)
    with pytest.raises(RuntimeError, match="value must be -1"):
        plan.set_variant("conv_wino_upz", 2)
    try:
        L.set_conv_wino_upz(2)
    finally:
        L.set_conv_wino_upz(-1)
