"""The SKIP variant of the Winograd kernel (csrc/conv_wino.hip, WinoSkipCfg): conv1 of an un-resampled decoder block COMPUTES
its residual -- the block's 1x1 skip projection -- on the matrix pipe in its epilogue instead of reading back what a
conv1x1_reg_kernel launch stored.  The projection is summed in that kernel's order (K = 2 steps over ascending channel pairs from
the matrix pipe's zero, bias afterwards), so the two paths must agree BIT FOR BIT, outputs and fused GroupNorm records alike:

  * op level, four shapes, with one tile per workgroup (this process) and with four (MCEDM_WINO_PER in a child process, as in
    tests/test_hip_wino_per.py: tile boundaries, first and last tile of a workgroup), the kernels named by the profiler;
  * the same runs against fp64 at the bar of tests/_tol.py (rtol 1e-4, atol 1e-5 x max|sample|);
  * one inference forward of the ch = 128, ch_mult (1, 1, 1, 1) network at 32 x 32: fold on == fold off, and with the fold on no
    conv1x1_reg_kernel launch is left.
The plain kernel's precondition (finite activations) holds here too; no test feeds Inf or NaN."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import mcedm_oracle as orc
from tests import _tol
from tests import _wino_fold as WF

pytestmark = pytest.mark.gpu
SKIP_KERNEL = "conv_wino_kernel<WinoSkipCfg<4>, false, true>"
PLAIN_KERNEL = "conv_wino_kernel<WinoCfg<4>, false, true>"


@pytest.fixture(scope="module")
def lib():
    import importlib
    L = importlib.import_module("m-cedm_amd.lib")
    L.load()
    return L


@pytest.fixture(scope="module")
def runs(lib, tmp_path_factory):
    """{1: this process (the default schedule: one tile per workgroup at these sizes), FORCED: the child}."""
    path = str(tmp_path_factory.mktemp("wino_fold") / "forced.npz")
    out = {1: WF.run_all(lib)}
    env = dict(os.environ, MCEDM_WINO_PER=str(WF.FORCED))
    r = subprocess.run([sys.executable, WF.__file__, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out[WF.FORCED] = dict(np.load(path))
    return out


@pytest.fixture(scope="module")
def refs():
    """fp64, computed once."""
    return {name: WF.case_reference(WF.case_inputs(name)) for name in WF.CASES}


@pytest.mark.parametrize("per", (1, WF.FORCED))
@pytest.mark.parametrize("name", list(WF.CASES))
def test_folded_projection_is_bit_equal_to_its_own_launch(runs, name, per):
    r = runs[per]
    total = WF.n_tiles(name)
    for key in ("on", "off"):                            # the schedule that ran, from every workgroup's record of the conv1 launch
        words = r[f"{name}/{key}/per"]
        assert (words[:total // per] == per).all() and (words[total // per:] == 0).all(), (name, key, per, words.tolist())
    on, off = set(r[f"{name}/on/names"].tolist()), set(r[f"{name}/off/names"].tolist())
    assert SKIP_KERNEL in on and "conv1x1_reg_kernel" not in on and len(on) == 1, on
    assert PLAIN_KERNEL in off and "conv1x1_reg_kernel" in off and SKIP_KERNEL not in off, off
    a, b = r[f"{name}/on/out"], r[f"{name}/off/out"]
    print(f"{name} per {per}: {int((a != b).sum())} of {a.size} outputs differ, max |d| {float(np.abs(a - b).max()):.3e}")
    assert np.array_equal(a, b)
    sa, sb = r[f"{name}/on/sums"], r[f"{name}/off/sums"]
    assert np.abs(sa).max() > 0 and np.array_equal(sa, sb), f"{name} per {per}: {int((sa != sb).sum())} of {sa.size} GroupNorm records differ"
    assert np.array_equal(a, runs[1][f"{name}/on/out"]), f"{name}: per {per} differs from per 1"


@pytest.mark.parametrize("per", (1, WF.FORCED))
@pytest.mark.parametrize("name", list(WF.CASES))
def test_folded_projection_vs_fp64(runs, refs, name, per):
    worst = _tol.close_per_entry(runs[per][f"{name}/on/out"], refs[name], what=f"{name} per {per}: folded conv1 vs fp64", time_dim=0)
    print(f"{name} per {per}: worst err / bound {worst:.3f}")


def test_inference_forward_with_the_fold_is_bit_equal_and_has_no_projection_launch(lib):
    cfg = orc.UNetConfig(ch=128, ch_mult=(1, 1, 1, 1), attn_resolutions=(), resolution=32)
    mk = lambda: lib.Plan(cfg.in_channels, cfg.cond_channels, cfg.out_ch, cfg.ch, cfg.ch_mult, cfg.num_res_blocks,
                          cfg.attn_resolutions, cfg.resolution)
    P = {k: v.cuda() for k, v in orc.make_params(cfg, 5).items()}
    x, cond = fx.randn("wino_fold/plan/x", 2, 2, 32, 32).cuda(), fx.randn("wino_fold/plan/c", 2, 2, 32, 32).cuda()
    sig = torch.tensor([0.5, 2.0]).cuda()
    got = {}
    for fold in (1, 0):
        plan = mk()
        plan.set_variant("conv_wino_fold", fold)
        packed = plan.pack(P)
        lib.prof_enable(True)
        try:
            D = plan.denoise(packed, x, sig, cond=cond)
            torch.cuda.synchronize()
            rows = {r["name"]: int(r["launches"]) for r in lib.prof_report()}
        finally:
            lib.prof_enable(False)
        got[fold] = (D.cpu(), rows)
    on, off = got[1][1], got[0][1]
    print("fold on:", on.get(SKIP_KERNEL, 0), "SKIP launches; fold off:", off.get("conv1x1_reg_kernel", 0), "projection launches")
    assert on.get("conv1x1_reg_kernel", 0) == 0 and on.get(SKIP_KERNEL, 0) > 0, on
    assert off.get("conv1x1_reg_kernel", 0) == on[SKIP_KERNEL] and off.get(SKIP_KERNEL, 0) == 0, off
    assert torch.equal(got[1][0], got[0][0]), f"{int((got[1][0] != got[0][0]).sum())} of {got[0][0].numel()} values differ"
