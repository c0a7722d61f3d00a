"""The Winograd kernels' epilogue (csrc/conv_wino.hip): one dispatch on the residual mode in front of straight-line loads -- the
half-resolution residual (RS_UP) without a copy behind every load, the double-resolution one (RS_DOWN) as a rolling window of
eight channels --, the record width tested once in front of the statistics, the 32-lane sums' last step in registers
(v_permlane16_swap_b32 instead of ds_bpermute_b32).  Same operations on the same values in the same order, so:

  1. outputs, signs of zeros and fused GroupNorm records equal conv_wino1_kernel's bit for bit (conv_wino1.hip is untouched and
     keeps half_sum32 and its own residual code): B = 3, 32 x 32, Cout = 128; residual none / same / RS_UP (source 16 x 16) /
     RS_DOWN (source 64 x 64); records of 4 and of 2 channels; activation on and off; Cin = 16 (one stage per tile: the one-stage
     trip), 32, 128 and 128 + 128 from two sources.  Every (residual, record width, activation) combination runs at Cin = 32, and
     across the other three Cin each residual mode meets three more of the four (record width, activation) pairs.  WinoCfg<2>
     (Cout = 64) and the split kernel (16 x 16, RS_DOWN from 32 x 32), which conv_wino1_kernel does not serve, are compared with
     it through zero-padded output channels / on the same shape, as in tests/test_hip_wino_addr.py.
  2. the four residual modes again with FOUR tiles per workgroup (MCEDM_WINO_PER = 4 in a child process, B = 2, 64 x 64: eight
     workgroups per sample, whole outputs compared, so a workgroup's first and last tile are both covered).
  3. the up-sampling form (16^2 -> 32^2) and the SKIP form (64 + 64 projection) against fp64 at the bar of tests/_tol.py; the
     worst fraction of the bar is printed next to the parent commit's (0.035 and 0.024) and may not exceed it: the operations
     are the same."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import _tol
from tests import _wino_epilogue as WE
from tests import _wino_per as WP

pytestmark = pytest.mark.gpu

B, H, W, COUT = 3, 32, 32, 128
CINS = {"cin16": (16, 0), "cin32": (32, 0), "cin128": (128, 0), "cin128x2": (128, 128)}
RC_ACT = [(4, 1), (2, 1), (4, 0), (2, 0)]
CASES = {}
for res in WE.RES_MODES:                     # Cin = 32: the full product
    for rc, act in RC_ACT:
        CASES[f"cin32_{res}_rc{rc}_act{act}"] = ("cin32", res, rc, act)
for ci, cin in enumerate(c for c in CINS if c != "cin32"):
    for ri, res in enumerate(WE.RES_MODES):
        for k in range(3):                   # three of the four (rc, act) pairs per (Cin, residual), rotating
            rc, act = RC_ACT[(ci + ri + k) % 4]
            CASES[f"{cin}_{res}_rc{rc}_act{act}"] = (cin, res, rc, act)
# the parent commit's worst error / bar of the two fp64 comparisons (tests/test_hip_wino_addr.py on that commit)
PARENT_UP_FRACTION, PARENT_SKIP_FRACTION = 0.035, 0.024


@pytest.fixture(scope="module")
def lib():
    import importlib
    L = importlib.import_module("m-cedm_amd.lib")
    L.load()
    return L


def assert_bits(name, a, ra, b, rb):
    print(f"{name}: {int((a != b).sum())} of {a.numel()} outputs differ, max |d| {float((a - b).abs().max()):.3e}; "
          f"{int((ra != rb).sum())} of {ra.numel()} record values differ")
    assert torch.isfinite(a).all() and torch.isfinite(ra).all() and rb.abs().max() > 0
    assert torch.equal(a, b)
    assert torch.equal(torch.signbit(a), torch.signbit(b))
    assert torch.equal(ra, rb)
    assert torch.equal(torch.signbit(ra), torch.signbit(rb))


@pytest.mark.parametrize("name", list(CASES))
def test_outputs_and_records_equal_the_one_wave_kernel(lib, name):
    cin, res, rc, act = CASES[name]
    Ca, Cb = CINS[cin]
    t = WE.make_inputs("wino_epilogue/" + name, B, Ca, Cb, COUT, H, W, act, res)
    a, ra, na = WE.launch(lib, t, COUT, act, res, rc)
    b, rb, nb = WE.launch(lib, t, COUT, act, res, rc, wino1=True)
    assert na == [f"conv_wino_kernel<WinoCfg<4>, false, {'true' if act else 'false'}>"], na
    assert len(nb) == 1 and nb[0].startswith("conv_wino1_kernel"), nb
    assert ra.shape == (B, 8, COUT // rc, 2)
    assert_bits(name, a, ra, b, rb)


@pytest.mark.parametrize("res", WE.RES_MODES)
@pytest.mark.parametrize("rc", [4, 2])
def test_64_channel_kernel_equals_the_one_wave_kernel(lib, res, rc):
    t = WE.make_inputs(f"wino_epilogue/c64_{res}", B, 32, 0, 64, H, W, 1, res)
    a, ra, na = WE.launch(lib, t, 64, 1, res, rc)
    b, rb, nb = WE.launch(lib, t, 64, 1, res, rc, wino1=True, pad_to=128)
    assert na == ["conv_wino_kernel<WinoCfg<2>, false, true>"], na
    assert len(nb) == 1 and nb[0].startswith("conv_wino1_kernel"), nb
    assert_bits(f"c64 {res} rc {rc}", a, ra, b, rb)


@pytest.mark.parametrize("res", ["none", "same", "down"])
def test_split_kernel_equals_the_one_wave_kernel(lib, res):
    t = WE.make_inputs(f"wino_epilogue/split_{res}", B, 64, 0, COUT, 16, 16, 1, res)
    a, ra, na = WE.launch(lib, t, COUT, 1, res, 4, split=True)
    b, rb, nb = WE.launch(lib, t, COUT, 1, res, 4, wino1=True)
    assert na == ["conv_wino_kernel<WinoSplitCfg, false, true>"], na
    assert len(nb) == 1 and nb[0].startswith("conv_wino1_kernel"), nb
    assert_bits(f"split {res}", a, ra, b, rb)


@pytest.fixture(scope="module")
def per4(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("wino_epilogue") / "per4.npz")
    r = subprocess.run([sys.executable, WE.__file__, path], env=dict(os.environ, MCEDM_WINO_PER="4"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return dict(np.load(path))


@pytest.mark.parametrize("res", WE.RES_MODES)
def test_four_tiles_per_workgroup_equal_the_one_wave_kernel(per4, res):
    Bp, _, _, Hp, Wp = WE.PER_SHAPE
    total = WP.n_tiles(Bp, Hp, Wp)
    for key in (res, res + "@wino1"):
        words = per4[key + "/per"]
        assert words.shape == (total,) and (words[:total // 4] == 4).all() and (words[total // 4:] == 0).all(), (key, words.tolist())
    assert [str(n) for n in per4[res + "/names"]] == ["conv_wino_kernel<WinoCfg<4>, false, true>"], per4[res + "/names"]
    assert str(per4[res + "@wino1/names"][0]).startswith("conv_wino1_kernel")
    a, ra = torch.from_numpy(per4[res + "/out"]), torch.from_numpy(per4[res + "/rec"])
    b, rb = torch.from_numpy(per4[res + "@wino1/out"]), torch.from_numpy(per4[res + "@wino1/rec"])
    assert_bits(f"per 4 {res}", a, ra, b, rb)


def activated64(x, coef):
    c = coef.double()
    return torch.nn.functional.silu((x.double() - c[..., 0, None, None]) * c[..., 1, None, None] + c[..., 2, None, None])


def test_up_sampling_form_vs_fp64(lib):
    tag = "wino_addr/up"                         # the inputs of tests/test_hip_wino_addr.py's case, whose fraction the parent's figure is
    x, coef = fx.randn(tag + "/xa", B, 64, 16, 16), WP.coef_table(tag, B, 64)
    w, b = fx.randn(tag + "/w", COUT, 64, 3, 3) / (64 * 9) ** 0.5, fx.randn(tag + "/b", COUT) * 0.1
    lib.prof_enable(True)
    try:
        out, _ = lib.op_conv_wino(WP.dev(x), None, lib.op_pack_conv_wino(WP.dev(w)), WP.dev(b), COUT, coef=WP.dev(coef), act=1, resample=WE.RS_UP,
                                  want_sums=True)
        torch.cuda.synchronize()
        names = sorted({r["name"] for r in lib.prof_report()})
    finally:
        lib.prof_enable(False)
    assert names == ["conv_wino_kernel<WinoCfg<4>, true, true, WinoUp<true>>"], names
    xu = torch.nn.functional.interpolate(activated64(x, coef), scale_factor=2, mode="nearest")
    ref = torch.nn.functional.conv2d(xu, w.double(), b.double(), padding=1)
    worst = _tol.close_per_entry(out.cpu(), ref, what="up-sampled Winograd conv 16^2 -> 32^2 vs fp64", time_dim=0)
    print(f"up-sampling form: worst err / bar {worst:.3f} (parent commit: {PARENT_UP_FRACTION})")
    assert round(worst, 3) <= PARENT_UP_FRACTION


def test_skip_form_vs_fp64(lib):
    tag, Cin, sa, sb = "wino_addr/skip128_64_64", 128, 64, 64      # the inputs of tests/test_hip_wino_addr.py's case, as above
    x, coef = fx.randn(tag + "/x", B, Cin, H, W), WP.coef_table(tag, B, Cin)
    w, b = fx.randn(tag + "/w", COUT, Cin, 3, 3) / (Cin * 9) ** 0.5, fx.randn(tag + "/b", COUT) * 0.1
    ws, bs = fx.randn(tag + "/ws", COUT, sa + sb, 1, 1) / (sa + sb) ** 0.5, fx.randn(tag + "/bs", COUT) * 0.1
    ska, skb = fx.randn(tag + "/ska", B, sa, H, W), fx.randn(tag + "/skb", B, sb, H, W)
    wpk, bpk = lib.op_pack_conv(WP.dev(w), WP.dev(b))
    swpk, sbpk = lib.op_pack_conv(WP.dev(ws), WP.dev(bs))
    lib.prof_enable(True)
    try:
        out, gsum = lib.op_conv_skip(WP.dev(x), wpk, lib.op_pack_conv_wino(WP.dev(w)), bpk, COUT, coef=WP.dev(coef), sk_xa=WP.dev(ska), sk_xb=WP.dev(skb),
                                     sk_wpk=swpk, sk_wfrag=lib.op_pack_conv_frag(WP.dev(ws)), sk_bias=sbpk, want_sums=True)
        torch.cuda.synchronize()
        names = sorted({r["name"] for r in lib.prof_report()})
    finally:
        lib.prof_enable(False)
    assert names == ["conv_wino_kernel<WinoSkipCfg<4>, false, true>"], names
    ref = torch.nn.functional.conv2d(activated64(x, coef), w.double(), b.double(), padding=1) + \
        torch.nn.functional.conv2d(torch.cat([ska, skb], 1).double(), ws.double(), bs.double())
    worst = _tol.close_per_entry(out.cpu(), ref, what="SKIP form 128 + (64 + 64) vs fp64", time_dim=0)
    print(f"SKIP form: worst err / bar {worst:.3f} (parent commit: {PARENT_SKIP_FRACTION})")
    assert round(worst, 3) <= PARENT_SKIP_FRACTION
    # its records (the statistics phase with the slots addressed inside it): sum and M2 of every 4-channel block of a tile vs fp64
    rec = gsum[:B * 8 * (COUT // 4) * 2].view(B, 8, COUT // 4, 2).cpu().double()
    blocks = ref.view(B, COUT // 4, 4, H // 8, 8, W // 16, 16).permute(0, 3, 5, 1, 2, 4, 6).reshape(B, 8, COUT // 4, -1)
    s64 = blocks.sum(-1)
    m64 = ((blocks - blocks.mean(-1, keepdim=True)) ** 2).sum(-1)
    es, em = float((rec[..., 0] - s64).abs().max()), float(((rec[..., 1] - m64).abs() / m64).max())
    print(f"SKIP form records: max |sum - fp64| {es:.3e} (512 values of |v| ~ 1.5), max relative M2 error {em:.3e}")
    # 512 values per record, each within the output bar (rtol 1e-4, atol 1e-5 at |v| < 8: 8.1e-4) -> the sum within 512 x that;
    # M2 ~ 512 var: relative error of the same order as the values' (1e-4) plus the fp32 sum's 512 eps
    assert es <= 512 * 8.1e-4 and em <= 1e-3
