"""The zero-position variant of the up-sampling Winograd kernel (csrc/conv_wino.hip, WinoUp): the input of an up block's conv0 is
the nearest 2x up-sampling of its source and tiles start on even pixels, so rows (and columns) 1 and 2 of every 4 x 4 input patch are
equal and the transformed input is exactly +0 at the seven Winograd positions with xi = 2 or nu = 2.  The variant does nothing for
them; every other product enters the same sum in the same order, so it must agree with the sixteen-position kernel BIT FOR BIT,
outputs and fused GroupNorm records alike:

  * op level (the variant, its positions alone on the old staging, and the sixteen-position kernel), seven cases (2 x 2 tiles, two
    sources, an odd chunk count, two output blocks, the 256-thread kernel, no activation, the RS_UP residual), with one tile per workgroup (this process) and with two where two divide the tiles per image (MCEDM_WINO_PER in
    a child process, as in tests/test_hip_wino_per.py: first and last tile of a workgroup, stages that cross a tile boundary), the
    kernels named by the profiler;
  * the "on" runs against fp64 at the bar of tests/_tol.py (rtol 1e-4, atol 1e-5 x max|sample|);
  * one inference forward of the ch = 128, ch_mult (1, 1, 1, 1) network at 32 x 32: variant on == off, the new kernel in the "on" arm
    only, one launch for each launch of the sixteen-position kernel in the "off" arm.
All inputs are finite (the variant's precondition: finite transformed weights); no test feeds Inf or NaN."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import mcedm_oracle as orc
from tests import _tol
from tests import _wino_upz as WU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import importlib
    L = importlib.import_module("m-cedm_amd.lib")
    L.load()
    return L


@pytest.fixture(scope="module")
def runs(lib, tmp_path_factory):
    """{1: this process (the default schedule: one tile per workgroup at these sizes), FORCED: the child}."""
    path = str(tmp_path_factory.mktemp("wino_upz") / "forced.npz")
    out = {1: WU.run_all(lib)}
    env = dict(os.environ, MCEDM_WINO_PER=str(WU.FORCED))
    r = subprocess.run([sys.executable, WU.__file__, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out[WU.FORCED] = dict(np.load(path))
    return out


@pytest.fixture(scope="module")
def refs():
    """fp64, computed once."""
    return {name: WU.case_reference(name, WU.case_inputs(name)) for name in WU.CASES}


@pytest.mark.parametrize("forced", (1, WU.FORCED))
@pytest.mark.parametrize("name", list(WU.CASES))
def test_zero_position_variant_is_bit_equal_to_sixteen_positions(runs, name, forced):
    r = runs[forced]
    total, per_img = WU.tiles(name)
    per = forced if per_img % forced == 0 else 1          # a forced count that does not divide leaves the default schedule
    for key, kernel in WU.kernels(name).items():          # the schedule that ran, from every workgroup's record; the kernel that ran
        words = r[f"{name}/{key}/per"]
        assert (words[:total // per] == per).all() and (words[total // per:] == 0).all(), (name, key, per, words.tolist())
        assert r[f"{name}/{key}/names"].tolist() == [kernel], (key, r[f"{name}/{key}/names"])
    b, sb = r[f"{name}/off/out"], r[f"{name}/off/sums"]
    assert np.abs(sb).max() > 0
    for key in ("on", "pos"):
        a, sa = r[f"{name}/{key}/out"], r[f"{name}/{key}/sums"]
        print(f"{name} per {per} {key}: {int((a != b).sum())} of {a.size} outputs differ, max |d| {float(np.abs(a - b).max()):.3e}")
        assert np.array_equal(a, b)
        assert np.array_equal(np.signbit(a), np.signbit(b))   # array_equal holds -0 == +0: the zeros' signs too
        assert np.array_equal(sa, sb), f"{name} per {per} {key}: {int((sa != sb).sum())} of {sa.size} GroupNorm records differ"
    assert np.array_equal(r[f"{name}/on/out"], runs[1][f"{name}/on/out"]), f"{name}: per {per} differs from per 1"


@pytest.mark.parametrize("forced", (1, WU.FORCED))
@pytest.mark.parametrize("name", list(WU.CASES))
def test_zero_position_variant_vs_fp64(runs, refs, name, forced):
    worst = _tol.close_per_entry(runs[forced][f"{name}/on/out"], refs[name], what=f"{name} forced {forced}: up-sampled conv vs fp64", time_dim=0)
    print(f"{name} forced {forced}: worst err / bound {worst:.3f}")


def test_inference_forward_with_the_variant_is_bit_equal_and_names_its_kernel(lib):
    cfg = orc.UNetConfig(ch=128, ch_mult=(1, 1, 1, 1), attn_resolutions=(), resolution=32)
    mk = lambda: lib.Plan(cfg.in_channels, cfg.cond_channels, cfg.out_ch, cfg.ch, cfg.ch_mult, cfg.num_res_blocks,
                          cfg.attn_resolutions, cfg.resolution)
    P = {k: v.cuda() for k, v in orc.make_params(cfg, 5).items()}
    x, cond = fx.randn("wino_upz/plan/x", 2, 2, 32, 32).cuda(), fx.randn("wino_upz/plan/c", 2, 2, 32, 32).cuda()
    sig = torch.tensor([0.5, 2.0]).cuda()
    k_on, k_off = "conv_wino_kernel<WinoCfg<4>, true, true, WinoUp<true>>", "conv_wino_kernel<WinoCfg<4>, true, true>"
    got = {}
    for flag in (1, 0):
        plan = mk()
        plan.set_variant("conv_wino_upz", flag)
        packed = plan.pack(P)
        lib.prof_enable(True)
        try:
            D = plan.denoise(packed, x, sig, cond=cond)
            torch.cuda.synchronize()
            rows = {r["name"]: int(r["launches"]) for r in lib.prof_report()}
        finally:
            lib.prof_enable(False)
        got[flag] = (D.cpu(), rows)
    on, off = got[1][1], got[0][1]
    print("variant on:", on.get(k_on, 0), "launches of the nine-position kernel; off:", off.get(k_off, 0), "of the sixteen-position kernel")
    # one launch per up block whose conv0 the Winograd kernel serves (32 x 32 outputs and larger)
    assert on.get(k_on, 0) >= 1 and on.get(k_off, 0) == 0, on
    assert off.get(k_off, 0) == on[k_on] and off.get(k_on, 0) == 0, off
    assert torch.equal(got[1][0], got[0][0]), f"{int((got[1][0] != got[0][0]).sum())} of {got[0][0].numel()} values differ"
