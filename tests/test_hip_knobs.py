"""GPU: the kernel variants that only an environment knob selects (tests/_knobs.py), each group of knobs in a child process of its
own (the library reads a knob once per process), held against fp64 at the bar of the default path's tests, with the profiler row
and variant ("name[variant]", tests/_knobs.py row_tokens) of the instantiation each case was written for, and bit for bit against the default path where INTEGRATION.md says "same bits".

The children run one after another, and after a child that ends with a nonzero status, a signal or a timeout NO further child is
started: a fault in one variant is not followed by more launches on the same card.  Every test of a group that did not run fails
with the name of the group that stopped the run.

As measured on an MI355X: the child's wall time (process start to exit, library load included) and the worst err / bar against fp64
over the group's cases (<= 1 passes):

    group            wall    worst err / bar
    attn_split0      2.2 s   a 0.8629 (T = 529, x6), dqkv 0.3503
    attn_split2      2.3 s   a 0.9866 (T = 576, x6), dqkv 0.9844 (T = 256, x6)
    attn_lds1        2.0 s   a 0.9411 (T = 529 on split<4>; lds<1>: 0.8985 at T = 516)
    attn_ldsmin      2.4 s   a 0.6902, dqkv 0.9847 (T = 256, x6)
    attn_ldsmin16    2.2 s   a 0.5594 (T = 20, x6), dqkv 0.1949
    attn_xcd0        2.1 s   a 0.7980, dqkv 0.9847; bit-equal to the default order
    c1_ni4           2.6 s   0.1416; bit-equal to NI = 2
    gn_twopass256    2.3 s   dxa 0.0029, dgamma 0.0062, dbeta 0.0073, dfilm 0.0040
    gn_twopass1024   2.7 s   dxa 0.0029, dgamma 0.0078, dbeta 0.0048, dfilm 0.0040
    wino_min256      2.1 s   0.2369 (WinoCfg<4>, two sources, 16 x 16); 8 x 16 stays on the split form

attn_split0's pairs are what this file found: under MCEDM_ATTN_SPLIT=0 the forward forms its scores in natural units at every T
and the backward recomputed them in units of log 2 from 128 tokens on.  dqkv on the x6 inputs, err / bar, before -> after the
backward took its units from the forward's own choice (csrc/common.hpp attn_fwd_kernel):

    T = 129 (direct<4>)  0.9298 -> 0.3223        T = 256 (lds)  1.6501 -> 0.3148
    T = 169 (direct<4>)  1.2113 -> 0.3503        T = 512 (lds)  1.5494 -> 0.2913
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from tests import _attn_bwd as AB
from tests import _knobs as K

pytestmark = pytest.mark.gpu

# seconds per child: three times the slowest child's measured wall time (2.7 s, the table above), rounded up
CHILD_TIMEOUT_S = 10


@pytest.fixture(scope="module")
def lib():
    import mcedm_amd  # noqa: F401
    from mcedm_amd import lib as L
    assert torch.cuda.is_available()
    L.load()
    return L


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """{group: its .npz as a dict}, plus "stopped": None or (group, why) of the child after which nothing more was started."""
    out = {"stopped": None}
    tmp = tmp_path_factory.mktemp("knobs")
    for name, (env, _) in K.GROUPS.items():
        path = str(tmp / f"{name}.npz")
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, K.__file__, name, path], env=dict(os.environ, **env), capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT_S)
            why = None if r.returncode == 0 else f"exit status {r.returncode}: {r.stderr[-1500:]}"
        except subprocess.TimeoutExpired:
            why = f"no result after {CHILD_TIMEOUT_S} s"
        print(f"child {name}: {time.time() - t0:.1f} s" + (f" -- {why}" if why else ""))
        if why:
            out["stopped"] = (name, why)
            break
        out[name] = dict(np.load(path))
    return out


@pytest.fixture(scope="module")
def defaults(lib, children):
    """The parent's default-path runs for the bit comparisons, computed once: {case key: {name: array}}.  After the children, and
    not at all after a child that stopped the run."""
    if children["stopped"]:
        pytest.fail(f"the run stopped at group {children['stopped'][0]}: nothing more is launched ({children['stopped'][1]})")
    out = {}
    for group in ("attn_xcd0", "c1_ni4"):
        for key in K.GROUPS[group][1]:
            out[key] = K.run_case(lib, key)
    return out


def of(children, group):
    if group not in children:
        pytest.fail(f"group {group} did not run: the run stopped at group {children['stopped'][0]} ({children['stopped'][1]})")
    return children[group]


def check_rows(case, rows):
    bad = K.rows_ok(case, rows)
    assert not bad, (bad, rows)


def attn_ratios(case, got, key):
    a64, g64 = K.attn_reference(case.shape, case.sub)
    r = {"a": AB.bar_ratio(got[key + "/a"], a64)}
    if case.kind == "attn_pair":
        dqkv = torch.from_numpy(got[key + "/dqkv"])
        assert bool(torch.isfinite(dqkv).all()), int((~torch.isfinite(dqkv)).sum())
        r["dqkv"] = AB.bar_ratio(AB.unpacked_qkv(dqkv, case.shape[1]), g64)
    return r


ALL = [(g, k) for g, (_, keys) in K.GROUPS.items() for k in keys]


@pytest.mark.parametrize("group,key", [(g, k) for g, k in ALL if g.startswith("attn")], ids=lambda v: v if "/" in v else "")
def test_attention_variant(children, defaults, group, key):
    got, case = of(children, group), K.CASES[key]
    check_rows(case, str(got[key + "/rows"]).split(";"))
    r = attn_ratios(case, got, key)
    print(f"{key}: rows {got[key + '/rows']}; err / bar vs fp64: " + ", ".join(f"{k} {v:.4f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
    if group == "attn_xcd0":
        # the block remap changes which workgroup computes what, not a bit of the result
        mine = defaults[key]
        assert str(mine[key + "/rows"]) == str(got[key + "/rows"])
        for name in ("a", "dqkv")[:len(r)]:
            assert np.array_equal(mine[f"{key}/{name}"], got[f"{key}/{name}"]), (name, float(np.abs(mine[f"{key}/{name}"] - got[f"{key}/{name}"]).max()))


@pytest.mark.parametrize("key", K.GROUPS["c1_ni4"][1])
def test_conv1x1_four_blocks_per_wave(children, defaults, key):
    got, case = of(children, "c1_ni4"), K.CASES[key]
    check_rows(case, str(got[key + "/rows"]).split(";"))
    ref = K.c1_reference64(case.shape)
    mine = defaults[key]
    assert K.c1_row(case.shape[3]) in str(mine[key + "/rows"]).split(";"), mine[key + "/rows"]
    for who, out in (("NI = 4", got[key + "/out"]), ("NI = 2", mine[key + "/out"])):
        err = (torch.from_numpy(out).double() - ref).abs()
        r = float((err / (1e-5 + 1e-4 * ref.abs())).max())
        print(f"{key}: {who}: err / bar vs fp64 {r:.4f}")
        assert r <= 1.0, (who, r)
    # csrc/conv1x1_reg.hip: "the two differ in the last bits of nothing: same sums"
    assert np.array_equal(got[key + "/out"], mine[key + "/out"]), float(np.abs(got[key + "/out"] - mine[key + "/out"]).max())


@pytest.mark.parametrize("key", K.GROUPS["wino_min256"][1])
def test_large_winograd_kernel_below_its_default_threshold(children, key):
    """tests/test_hip_wino.py's bar: rtol 1e-4, atol 1e-5."""
    got, case = of(children, "wino_min256"), K.CASES[key]
    check_rows(case, str(got[key + "/rows"]).split(";"))
    ref = K.wino_reference64(case.shape)
    out = torch.from_numpy(got[key + "/out"]).double()
    assert out.shape == ref.shape and bool(torch.isfinite(out).all())
    r = float(((out - ref).abs() / (1e-5 + 1e-4 * ref.abs())).max())
    print(f"{key}: rows {got[key + '/rows']}; err / bar vs fp64 {r:.4f}")
    assert r <= 1.0, r


@pytest.mark.parametrize("group,key", [(g, k) for g, k in ALL if g.startswith("gn_")], ids=lambda v: v if "/" in v else "")
def test_groupnorm_backward_two_pass_kernel(children, group, key):
    got, case = of(children, group), K.CASES[key]
    check_rows(case, str(got[key + "/rows"]).split(";"))
    ref = K.gn_reference64(case.shape)
    r = {}
    for name in K.GN_OUT:
        assert (ref[name] is None) == (f"{key}/{name}" not in got), name
        if ref[name] is not None:
            r[name] = AB.bar_ratio(got[f"{key}/{name}"], ref[name])
    print(f"{key}: rows {got[key + '/rows']}; err / bar vs fp64: " + ", ".join(f"{k} {v:.4f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
    if len(case.shape) > 10:
        assert int(got[key + "/sync_left"]) == 0, "the exchange area must be left zero"


def test_every_group_ran(children):
    assert children["stopped"] is None, children["stopped"]
    assert [g for g in K.GROUPS if g in children] == list(K.GROUPS)
